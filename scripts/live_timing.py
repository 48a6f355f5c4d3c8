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


def med(rows, key, lo=9):
    return round(float(np.median([r[key] for r in rows if r["windows"] >= lo])), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "live_timing_30s.json"))
    a = ap.parse_args()
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    dev = torch.device("cuda:0")
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=dev,
                            seg_state=turn_taking_state_dict(get_seg_config("wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    x = first_channel_16k(str(ROOT / "tests" / "golden" / "EN2002a_30s.wav"))
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
