"""The matching step of the Resegmentation pipeline at the 4 h shape (17 991 windows of 399 frames, S = 4 local speakers, a
hypothesis of K = 8 speakers), in one process on one device: dzn_match_counts alone (HIP events around the call, median of
`--reps` after two untimed calls), the whole postprocess.match_counts_device call (upload of the hypothesis and of the rows,
launch, download of the counts; host clock), and the host loop of postprocess.assign_windows (float32 division and one
scipy.optimize.linear_sum_assignment per window; host clock).  For the record only: nothing is compared with a bound.

    timeout -k 10 300 python scripts/reseg_timing.py            # -> profiles/reseg_timing_4h.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "reseg_timing_4h.json"))
    a = ap.parse_args()
    from diarizen_amd import _lib
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import assign_windows, match_counts_device, match_counts_host, receptive_field, reference_rows
    lib = _lib.load()
    dev = torch.device("cuda:0")
    Cn, L, S, K = 17991, 399, 4, 8
    n = max(K, S)
    g = np.random.default_rng(11)
    tog = g.random((Cn, L, S)) < 0.03
    tog[:, 0, :] = g.random((Cn, S)) < 0.4
    seg = (np.cumsum(tog, axis=1) % 2).astype(np.uint8)
    rows = reference_rows(Cn, SlidingWindow(start=0.0, duration=8.0, step=0.8), receptive_field())
    Tr = int(rows[-1]) + L - 25
    ref = (np.cumsum(g.random((Tr, K)) < 0.01, axis=0) % 2).astype(np.uint8)
    seg_t, ref_t = torch.from_numpy(seg).to(dev), torch.from_numpy(ref).to(dev)
    row_t = torch.from_numpy(rows).to(dev)
    out = torch.empty((Cn, n, n), device=dev, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = torch.cuda.current_stream(dev)
    times = []
    for _ in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        _lib.check(lib.dzn_match_counts(p(seg_t), p(ref_t), Cn, L, S, Tr, K, p(row_t), 0, L, p(out), C.c_void_p(st.cuda_stream)),
                   None, "dzn_match_counts")
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    counts = out.cpu().numpy()
    assert np.array_equal(counts[:64], match_counts_host(seg[:64], ref, rows[:64], 0, L, K))
    whole = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        match_counts_device(seg_t, ref, rows, 0, L, K)
        whole.append((time.perf_counter() - t0) * 1e3)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        assign_windows(counts, L, S)
        host.append((time.perf_counter() - t0) * 1e3)
    import scipy
    res = {"shape": {"windows": Cn, "frames": L, "local_speakers": S, "hypothesis_speakers": K, "reference_rows": Tr},
           "device": torch.cuda.get_device_name(dev), "scipy": scipy.__version__, "numpy": np.__version__,
           "dzn_match_counts_ms": {"median": round(float(np.median(times[2:])), 4), "min": round(float(np.min(times[2:])), 4),
                                   "reps": a.reps},
           "match_counts_device_ms": {"median": round(float(np.median(whole)), 3), "all": [round(t, 3) for t in whole]},
           "assign_windows_ms": {"median": round(float(np.median(host)), 2), "all": [round(t, 2) for t in host]}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
