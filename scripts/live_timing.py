"""What one feed of a live diarization session (diarizen_amd/live.py, LiveDiarization) costs once a new window is complete,
beside what pipeline.stream's StreamingSession does at the same point: on tests/golden/EN2002a_30s.wav (wavlm-large-s80, 8 s
windows at a 0.8 s step, 28 windows + a zero-padded 29th, seeded weights, delta_new 0.2), fed in 0.8 s chunks so that every
feed after the first 8 s completes exactly one window.

  * LiveDiarization.feed: wall clock of the whole call and of its three parts — the window through the engine with its
    download (_compute, which contains the online assignment, timed separately), and the range call with its download;
  * StreamingSession: the same window through the engine (_compute) and one refresh (_annotate: concatenate everything so far,
    upload all decisions, count, cluster, reconstruct) after the same number of windows.

Host wall clock (every part ends in a device-to-host copy), median over the feeds of windows 9 .. 28 after a warm-up pass.

    timeout -k 10 600 python scripts/live_timing.py        # -> profiles/live_timing_30s.json

With --feed-format (repeatable: ENCODING:RATE:CHANNELS, e.g. ulaw:8000:2) the script measures the ingest instead: the same
30 s through pipeline.open_live in 20 ms packets, once as float32 at 16 kHz (the feed every session had before feed_format)
and once per format given (resampled on the host to that rate and encoded; a second channel is the first delayed by 0.5 s;
the session hears channel 0) — the host time of one feed() that completes no window (staging, upload, and for a stored format
the one dzn_resample / dzn_decode launch), of one that completes a window, and the time from the last feed to the end of
finish().  The passes alternate (float32, format 1, format 2, float32, ...) after a warm-up of each, `--repeats` times; every
figure is given per repeat, so the spread can be read off.

    timeout -k 10 900 python scripts/live_timing.py --feed-format ulaw:8000:2 --feed-format s16:48000:1
                                                          # -> profiles/live_feed_timing_30s.json
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def live_pass(pipe, chunks):
    sess = pipe.open_live(sess_name="timing", delta_new=0.2, max_seconds=60.0)
    clocks = {"compute": Clock(sess, "_compute"), "assign": Clock(sess.speakers, "assign"), "range": Clock(sess, "_advance")}
    rows = []
    for c in chunks:
        before = {k: v.total for k, v in clocks.items()}
        done = sess.done
        t = time.perf_counter()
        sess.feed(c)
        dt = time.perf_counter() - t
        if sess.done == done + 1:
            rows.append(dict({k: 1e3 * (v.total - before[k]) for k, v in clocks.items()}, feed=1e3 * dt, windows=sess.done))
    sess.finish()
    return rows, sess.num_speakers


def session_pass(pipe, chunks):
    from diarizen_amd.streaming import StreamingSession
    sess = StreamingSession(pipe, "timing", max_seconds=60.0, refresh_s=None)
    rows = []
    for c in chunks:
        done = sess.done
        t = time.perf_counter()
        sess.feed(c)
        t1 = time.perf_counter()
        if sess.done == done + 1:
            sess._annotate()
            rows.append({"compute": 1e3 * (t1 - t), "refresh": 1e3 * (time.perf_counter() - t1), "windows": sess.done})
    sess.finish()
    return rows


def encode_feed(x16, spec: str):
    """ENCODING:RATE:CHANNELS -> (FeedFormat hearing channel 0, the 30 s as 20 ms packets of bytes in that format)"""
    import audioop
    from diarizen_amd.audio import FeedFormat, resample
    enc, rate, ch = spec.split(":")
    rate, ch = int(rate), int(ch)
    x = x16 if rate == 16000 else resample(x16, 16000, rate)
    cols = [np.concatenate([np.zeros(c * rate // 2, dtype=np.float32), x[:len(x) - c * rate // 2]]) for c in range(ch)]
    pcm = np.clip(np.rint(np.stack(cols, axis=1) * 32768.0), -32768, 32767).astype("<i2")
    if enc == "s16":
        body = pcm.tobytes()
    elif enc in ("ulaw", "alaw"):
        body = (audioop.lin2ulaw if enc == "ulaw" else audioop.lin2alaw)(pcm.tobytes(), 2)
    elif enc == "f32":
        body = np.stack(cols, axis=1).astype("<f4").tobytes()
    else:
        raise SystemExit(f"--feed-format: s16, ulaw, alaw or f32, not {enc!r}")
    fmt = FeedFormat(rate, enc, channels=ch, channel=0)
    size = rate // 50 * fmt.frame_bytes
    return fmt, [body[i:i + size] for i in range(0, len(body), size)]


def packet_pass(pipe, packets, fmt):
    """one live session over the packets -> ms: median feed without / with a new window, last feed -> finish() returned"""
    sess = pipe.open_live(sess_name="timing", delta_new=0.2, max_seconds=60.0, feed_format=fmt)
    quiet, window = [], []
    for p in packets:
        done = sess.done
        t = time.perf_counter()
        sess.feed(p)
        dt = 1e3 * (time.perf_counter() - t)
        (window if sess.done > done else quiet).append(dt)
    t = time.perf_counter()
    sess.finish()
    fin = 1e3 * (time.perf_counter() - t)
    return {"feed_ms_no_window": round(float(np.median(quiet)), 4), "feed_ms_no_window_p95": round(float(np.percentile(quiet, 95)), 4),
            "feed_ms_new_window": round(float(np.median(window)), 3), "finish_ms": round(fin, 3), "feeds": len(packets),
            "uploads": sess.stats["uploads"]}


def feed_format_main(a, pipe, x, dev):
    feeds = {"f32:16000:1 (no feed_format)": (None, [x[i:i + 320] for i in range(0, len(x), 320)])}
    for spec in a.feed_format:
        feeds[spec] = encode_feed(x, spec)
    for fmt, packets in feeds.values():           # warm-up: allocator, kernels, scipy, the filter bank
        packet_pass(pipe, packets, fmt)
    runs = {k: [] for k in feeds}
    for _ in range(a.repeats):
        for k, (fmt, packets) in feeds.items():
            runs[k].append(packet_pass(pipe, packets, fmt))
    return {"workload": "tests/golden/EN2002a_30s.wav through pipeline.open_live in 20 ms packets, wavlm_large_s80_md, 8 s windows, "
                        "step 0.8 s, seeded weights; host wall clock in ms, one entry per repeat, passes alternating",
            "device": torch.cuda.get_device_name(dev), "runs": runs}


def med(rows, key, lo=9):
    return round(float(np.median([r[key] for r in rows if r["windows"] >= lo])), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/live_timing_30s.json (live_feed_timing_30s.json with --feed-format)")
    ap.add_argument("--feed-format", action="append", default=[], metavar="ENCODING:RATE:CHANNELS",
                    help="measure the ingest in 20 ms packets: float32 at 16 kHz beside each format given")
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    if a.out is None:
        a.out = str(ROOT / "profiles" / ("live_feed_timing_30s.json" if a.feed_format else "live_timing_30s.json"))
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    dev = torch.device("cuda:0")
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=dev,
                            seg_state=turn_taking_state_dict(get_seg_config("wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    x = first_channel_16k(str(ROOT / "tests" / "golden" / "EN2002a_30s.wav"))
    if a.feed_format:
        res = feed_format_main(a, pipe, x, dev)
        pipe.close()
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
        return
    chunks = [x[i:i + 12800] for i in range(0, len(x), 12800)]
    live_pass(pipe, chunks)                       # warm-up: allocator, kernels, scipy
    session_pass(pipe, chunks)
    live, nspk = live_pass(pipe, chunks)
    sess = session_pass(pipe, chunks)
    res = {"workload": "tests/golden/EN2002a_30s.wav in 0.8 s chunks, wavlm_large_s80_md, 8 s windows, step 0.8 s, seeded weights; "
                       "host wall clock in ms, median over the feeds that complete windows 9 .. 28",
           "device": torch.cuda.get_device_name(dev), "live_speakers": nspk,
           "live_feed_ms": {"whole_feed": med(live, "feed"), "window_forward_and_download": round(med(live, "compute") - med(live, "assign"), 3),
                            "online_assignment": med(live, "assign"), "range_call_and_download": med(live, "range")},
           "live_range_ms_at_windows": {str(r["windows"]): round(r["range"], 3) for r in live if r["windows"] in (9, 18, 28)},
           "streaming_session_ms": {"window_forward_and_download": med(sess, "compute"), "refresh": med(sess, "refresh")},
           "streaming_session_refresh_ms_at_windows": {str(r["windows"]): round(r["refresh"], 3) for r in sess
                                                       if r["windows"] in (9, 18, 28)}}
    pipe.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
