"""What a live hub (diarizen_amd/hub.py, pipeline.open_hub) sustains beside the same sessions opened one by one: N sessions of
a 30 s 8 kHz two-channel mu-law call (tests/golden/EN2002a_30s.wav resampled and encoded; channel 1 is channel 0 delayed by
0.5 s; the sessions hear channel 0), every session delivering a 20 ms packet (320 bytes) per round.

  * hub: every session feeds its packet (host only), then ONE hub.tick() per round; all sessions finish, one last tick;
  * round robin: N pipeline.open_live sessions fed one after the other per round, then finished one after the other — what the
    sessions cost without a hub.

Per N and form, `--repeats` passes after a warm-up pass of each, alternating (hub, round robin, hub, ...): wall time of the
whole pass, sustained sessions x real time (N x 30 s / wall time), wall time per round (median and 95th percentile over the
rounds of a pass), and for the hub the host time spent in its parts (upload + ingest launch, forwards incl. the gather, the
one D2H, the sessions' host labelling and range calls).  The medians over the repeats and their spread (min .. max) are
reported, every repeat is listed.  A separate pass per form with the library's profiler on counts the device launches of
the library's kernels per round (torch's own copies and fills are not counted).

    timeout -k 10 1100 python scripts/hub_timing.py        # -> profiles/hub_ticks.json
"""
from __future__ import annotations

import argparse
import audioop
import copy
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PACKET = 320                                        # 20 ms of 8 kHz two-channel mu-law
DELTA = 0.2


class Clock:
    """wraps a bound method and adds up its wall-clock time"""

    def __init__(self, obj, name):
        self.fn, self.total = getattr(obj, name), 0.0
        setattr(obj, name, self)

    def __call__(self, *a, **k):
        t = time.perf_counter()
        try:
            return self.fn(*a, **k)
        finally:
            self.total += time.perf_counter() - t


def the_call(seconds: float):
    from _stream_cases import samples
    from diarizen_amd.audio import resample
    x8 = resample(samples(int(seconds * 16000))[0], 16000, 8000)
    x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)
    body = audioop.lin2ulaw(np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes(), 2)
    return [body[i:i + PACKET] for i in range(0, len(body), PACKET)]


def hub_pass(pipe, fmt, packets, N, count_launches=False):
    from diarizen_amd import _lib
    hub = pipe.open_hub(max_sessions=N, max_seconds=60.0)
    sessions = [hub.open(f"call-{i}", delta_new=DELTA, feed_format=fmt) for i in range(N)]
    clocks = {"upload_ingest": Clock(hub, "_upload"), "forward": Clock(hub, "_forward")}
    host = [Clock(s, "_take") for s in sessions]
    rng = [Clock(s, "_advance") for s in sessions]
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
               parts_s=dict({k: c.total for k, c in clocks.items()}, labelling=sum(c.total for c in host),
                            range_calls=sum(c.total for c in rng)),
               speakers=sessions[0].num_speakers, frames=len(sessions[0].committed_count))
    if count_launches:
        out["library_launches"] = launches
    hub.close()
    return out, rounds


def robin_pass(pipe, fmt, packets, N, count_launches=False):
    from diarizen_amd import _lib
    sessions = [pipe.open_live(sess_name=f"call-{i}", delta_new=DELTA, max_seconds=60.0, feed_format=fmt) for i in range(N)]
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
        rounds.append(time.perf_counter() - t)
        if count_launches and r % 25 == 24:
            launches += sum(e["launches"] for e in _lib.profile_collect())
    for s in sessions:
        s.finish()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if count_launches:
        launches += sum(e["launches"] for e in _lib.profile_collect())
        _lib.profile_enable(False)
    out = dict(wall_s=wall, rounds=len(rounds) + 1, windows=sum(s.stats["windows"] for s in sessions),
               forwards=sum(s.stats["launches"] for s in sessions), uploads=sum(s.stats["uploads"] for s in sessions),
               range_calls=sum(s.stats["range_calls"] for s in sessions), speakers=sessions[0].num_speakers,
               frames=len(sessions[0].committed_count))
    if count_launches:
        out["library_launches"] = launches
    del sessions
    return out, rounds


def summary(passes, seconds, N):
    walls = [p[0]["wall_s"] for p in passes]
    rate = [N * seconds / w for w in walls]
    med = [1e3 * statistics.median(p[1]) for p in passes]
    p95 = [1e3 * float(np.percentile(p[1], 95)) for p in passes]
    sp = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v), repeats=[round(x, 4) for x in v])      # noqa: E731
    return dict(wall_s=sp(walls), sessions_x_realtime=sp(rate), round_ms_median=sp(med), round_ms_p95=sp(p95),
                passes=[p[0] for p in passes])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hub_ticks.json"))
    a = ap.parse_args()
    from diarizen_amd.audio import FeedFormat
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    pipe = DiariZenPipeline(None, None, config=cfg, device=torch.device("cuda:0"), seg_state=turn_taking_state_dict(
        get_seg_config("wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    fmt = FeedFormat(8000, "ulaw", channels=2, channel=0)
    packets = the_call(a.seconds)
    result = dict(call=dict(seconds=a.seconds, rate=8000, channels=2, encoding="ulaw", packet_bytes=PACKET, packets=len(packets)),
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
        hl, rl = hub_pass(pipe, fmt, packets, N, True)[0], robin_pass(pipe, fmt, packets, N, True)[0]
        h["library_launches_per_round"] = hl["library_launches"] / hl["rounds"]
        r["library_launches_per_round"] = rl["library_launches"] / rl["rounds"]
        gain = h["sessions_x_realtime"]["median"] / r["sessions_x_realtime"]["median"]
        apart = h["sessions_x_realtime"]["min"] > r["sessions_x_realtime"]["max"]
        result["sessions"][str(N)] = dict(hub=h, round_robin=r, hub_over_round_robin=gain, beyond_the_spread=bool(apart))
        print(f"N={N}: hub {h['sessions_x_realtime']['median']:.1f} x real time ({h['sessions_x_realtime']['min']:.1f} .. "
              f"{h['sessions_x_realtime']['max']:.1f}), round robin {r['sessions_x_realtime']['median']:.1f} "
              f"({r['sessions_x_realtime']['min']:.1f} .. {r['sessions_x_realtime']['max']:.1f}); round median "
              f"{h['round_ms_median']['median']:.3f} ms vs {r['round_ms_median']['median']:.3f} ms; library launches per round "
              f"{h['library_launches_per_round']:.1f} vs {r['library_launches_per_round']:.1f}", flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")       # after every N: a partial file survives a time limit
    pipe.close()


if __name__ == "__main__":
    main()
