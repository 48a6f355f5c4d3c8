"""What a live hub sustains with ARRAY feeds (diarizen_amd/hub.py, csrc/beamform_many.hip) beside the same rooms
opened one by one: N rooms of a 4-microphone 16 kHz int16 feed (tests/golden/EN2002a_30s.wav as delayed copies plus noise, the
`arrays` fixture of tests/test_beamform_live_gpu.py), every room delivering a 20 ms packet (2560 bytes) per round.

  * hub: pipeline.open_hub(array_channels=4); every room feeds its packet (host only), then ONE hub.tick() per round;
  * round robin: N pipeline.open_live sessions fed one after the other per round — existing code, one dzn_beamform_feed per
    planned call and room: the baseline is not the code under test.

Per N and form, a warm-up pass of each, then `--repeats` alternating passes (scripts/hub_timing.py's passes and summary): wall
time, sustained sessions x real time, wall time per round; the medians over the repeats and their spread are reported and every
repeat is listed.  A separate pass per form with the library's profiler on counts the library's launches per round, and a
separate hub pass brackets every wave — the upload and its launch set — with events on the copy stream for its device time.

    timeout -k 10 1100 python scripts/hub_array_timing.py        # -> profiles/hub_array_ticks.json
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hub_timing import DELTA, Clock, robin_pass, summary  # noqa: E402

PACKET = 2560                                       # 20 ms of 16 kHz four-channel int16
DELAYS = (0, 5, -12, 30)


def the_room(seconds: float):
    from _stream_cases import samples
    from testkit import beamform_ref as R
    x = R.delayed_copies(samples(int(seconds * 16000))[0], DELAYS, 0.002, 17)
    body = np.clip(np.rint(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()
    return [body[i:i + PACKET] for i in range(0, len(body), PACKET)]


def slot_bytes(N: int) -> int:
    return max(1 << 20, N << 17)


def hub_pass(pipe, fmt, packets, N, count_launches=False, time_waves=False):
    from diarizen_amd import _lib
    # a call re-uploads 2 hop + max_lag frames of history beside its new frames (about 100 KB here): the slot is sized so that
    # the calls of all N rooms, whose blocks complete in the same round, make ONE wave
    hub = pipe.open_hub(max_sessions=N, max_seconds=60.0, slot_bytes=slot_bytes(N), array_channels=fmt.channels,
                        array_rate=fmt.rate)
    sessions = [hub.open(f"room-{i}", delta_new=DELTA, feed_format=fmt) for i in range(N)]
    clocks = {"waves": Clock(hub, "_upload_wave"), "forward": Clock(hub, "_forward")}
    events = []
    if time_waves:
        run = hub._upload_wave

        def timed(up, t):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(hub.copy_stream)
            run(up, t)
            b.record(hub.copy_stream)
            events.append((a, b, len(up.desc)))

        hub._upload_wave = timed
    launches = 0
    if count_launches:
        _lib.profile_enable(True)
        _lib.profile_collect()
    torch.cuda.synchronize()
    rounds = []
    t0 = time.perf_counter()
    for r, p in enumerate(packets):
        t = time.perf_counter()
        for s in sessions:
            s.feed(p)
        hub.tick()
        rounds.append(time.perf_counter() - t)
        if count_launches and r % 25 == 24:
            launches += sum(e["launches"] for e in _lib.profile_collect())
    for s in sessions:
        s.finish()
    hub.tick()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if count_launches:
        launches += sum(e["launches"] for e in _lib.profile_collect())
        _lib.profile_enable(False)
    out = dict(wall_s=wall, rounds=len(rounds) + 1, stats=dict(hub.stats["total"]),
               parts_s={k: c.total for k, c in clocks.items()}, speakers=sessions[0].num_speakers,
               frames=len(sessions[0].committed_count))
    if count_launches:
        out["library_launches"] = launches
    if time_waves:
        ms = [a.elapsed_time(b) for a, b, _ in events]
        out["wave_device_ms"] = dict(waves=len(ms), calls_per_wave=statistics.median(n for _, _, n in events),
                                     median=statistics.median(ms), min=min(ms), max=max(ms))
    hub.close()
    return out, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hub_array_ticks.json"))
    a = ap.parse_args()
    from diarizen_amd.audio import Beamform, FeedFormat
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    pipe = DiariZenPipeline(None, None, config=cfg, device=torch.device("cuda:0"), seg_state=turn_taking_state_dict(
        get_seg_config("wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    fmt = FeedFormat(16000, "s16", channels=4, channel=Beamform(causal=True))
    packets = the_room(a.seconds)
    hop, max_lag, _ = fmt.channel.plan(fmt.rate, fmt.channels)
    result = dict(room=dict(seconds=a.seconds, rate=16000, channels=4, encoding="s16", packet_bytes=PACKET, packets=len(packets),
                            hop=hop, max_lag=max_lag),
                  model="wavlm_large_s80_md, seeded weights, 8 s windows at a 0.8 s step, batch_size 64, delta_new 0.2",
                  device=torch.cuda.get_device_name(0), repeats=a.repeats, sessions={})
    for N in a.sessions:
        hub_pass(pipe, fmt, packets, N)                                 # warm-up of each form
        robin_pass(pipe, fmt, packets, N)
        hubs, robins = [], []
        for k in range(a.repeats):
            hubs.append(hub_pass(pipe, fmt, packets, N))
            robins.append(robin_pass(pipe, fmt, packets, N))
            print(f"  N={N} repeat {k}: hub {hubs[-1][0]['wall_s']:.2f} s, round robin {robins[-1][0]['wall_s']:.2f} s", flush=True)
        assert hubs[0][0]["frames"] == robins[0][0]["frames"] and hubs[0][0]["speakers"] == robins[0][0]["speakers"]
        h, r = summary(hubs, a.seconds, N), summary(robins, a.seconds, N)
        hl, rl = hub_pass(pipe, fmt, packets, N, count_launches=True)[0], robin_pass(pipe, fmt, packets, N, True)[0]
        h["library_launches_per_round"] = hl["library_launches"] / hl["rounds"]
        r["library_launches_per_round"] = rl["library_launches"] / rl["rounds"]
        h["wave_device_ms"] = hub_pass(pipe, fmt, packets, N, time_waves=True)[0]["wave_device_ms"]
        gain = h["sessions_x_realtime"]["median"] / r["sessions_x_realtime"]["median"]
        apart = h["sessions_x_realtime"]["min"] > r["sessions_x_realtime"]["max"]
        h["slot_bytes"] = slot_bytes(N)
        result["sessions"][str(N)] = dict(hub=h, round_robin=r, hub_over_round_robin=gain, beyond_the_spread=bool(apart))
        print(f"N={N}: hub {h['sessions_x_realtime']['median']:.1f} x real time ({h['sessions_x_realtime']['min']:.1f} .. "
              f"{h['sessions_x_realtime']['max']:.1f}), round robin {r['sessions_x_realtime']['median']:.1f} "
              f"({r['sessions_x_realtime']['min']:.1f} .. {r['sessions_x_realtime']['max']:.1f}); round median "
              f"{h['round_ms_median']['median']:.3f} ms vs {r['round_ms_median']['median']:.3f} ms; library launches per round "
              f"{h['library_launches_per_round']:.1f} vs {r['library_launches_per_round']:.1f}; wave "
              f"{h['wave_device_ms']['median']:.3f} ms ({h['wave_device_ms']['min']:.3f} .. {h['wave_device_ms']['max']:.3f}) "
              f"for {h['wave_device_ms']['calls_per_wave']} calls", flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")       # after every N: a partial file survives a time limit
    pipe.close()


if __name__ == "__main__":
    main()
