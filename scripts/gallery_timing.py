"""What the device gallery search (csrc/gallery.hip, ops.GalleryState) sustains on one MI355X: 2^20 seeded random rows x 256
(1 GiB of fp32, four times the Infinity Cache), Q in {1, 16, 64} queries, top_n = 16.

Per Q: `--warmup` searches, then `--repeats` searches, each timed with HIP events around its launches only (the scans and the
merges of all query groups; the upload of the queries and the copies of the results are outside — dzn_gallery_last_launch_ms).
Reported: the median, the spread (min .. max), the gallery bytes per second of the median (rows x dim x 4 bytes x sweeps, one
sweep per query group of `query_group` queries; and the same for ONE sweep, the figure that compares with the in-order HBM
sweep of MI355X: 6.0-6.1 TB/s for a 1.2 GB table) and the share of the last merge.  The aim is at least half of that rate at
Q = 16; it is an aim, not a test.

For the record, the only way to these numbers before: ops.cdist_cosine(gallery, queries) at 2^17 rows (both operands uploaded
per call, float64, the full matrix back), host wall time around the blocking call.

    timeout -k 10 500 python scripts/gallery_timing.py        # -> profiles/gallery_scan.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

HBM_SWEEP_TBS = (6.0, 6.1)          # measured in-order sweep of a 1.2 GB table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--top-n", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cdist-rows", type=int, default=1 << 17)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gallery_scan.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gallery_timing needs a HIP device: nothing is measured without one")
    from diarizen_amd import ops
    rng = np.random.default_rng(0)
    g = ops.GalleryState(a.dim, a.rows, 0)
    chunk = 1 << 16
    head = None
    for r0 in range(0, a.rows, chunk):
        block = rng.standard_normal((min(chunk, a.rows - r0), a.dim), dtype=np.float32)
        if head is None:
            head = block[:a.cdist_rows].copy() if a.cdist_rows <= chunk else None
        g.put(r0, block)
    gallery_bytes = a.rows * a.dim * 4
    result = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "dim": a.dim, "gallery_bytes": gallery_bytes,
              "top_n": a.top_n, "tile_rows": g.tile_rows, "sweep_rows": g.sweep_rows, "query_group": g.query_group,
              "warmup": a.warmup, "repeats": a.repeats, "hbm_in_order_sweep_TBs": list(HBM_SWEEP_TBS),
              "timing": "HIP events around the launches of one search (scans + merges); median over the repeats", "Q": {}}
    for Q in (1, 16, 64):
        q = rng.standard_normal((Q, a.dim), dtype=np.float32)
        for _ in range(a.warmup):
            g.search(q, a.top_n)
        ms, merge = [], []
        for _ in range(a.repeats):
            g.search(q, a.top_n)
            t, m = g.last_launch_ms()
            ms.append(t)
            merge.append(m)
        med = statistics.median(ms)
        sweeps = -(-Q // g.query_group)
        result["Q"][str(Q)] = {
            "sweeps": sweeps, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "last_merge_ms_median": statistics.median(merge),
            "gallery_TBs": gallery_bytes * sweeps / (med * 1e-3) / 1e12,
            "share_of_hbm_sweep": gallery_bytes * sweeps / (med * 1e-3) / 1e12 / HBM_SWEEP_TBS[0],
            "flop_per_s_T": 2.0 * a.rows * a.dim * Q / (med * 1e-3) / 1e12, "ms_all": ms}
        print(f"Q {Q:3d}: {med:.3f} ms ({min(ms):.3f} .. {max(ms):.3f}), {result['Q'][str(Q)]['gallery_TBs']:.2f} TB/s of gallery, "
              f"last merge {statistics.median(merge):.3f} ms", flush=True)
    g.close()
    # the parent's only way to these numbers
    n = a.cdist_rows
    e = head if head is not None else np.random.default_rng(1).standard_normal((n, a.dim), dtype=np.float32)
    cd = {}
    for Q in (1, 16, 64):
        c = rng.standard_normal((Q, a.dim)).astype(np.float64)
        ops.cdist_cosine(e, c, device=0)
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            ops.cdist_cosine(e, c, device=0)
            ts.append((time.perf_counter() - t) * 1e3)
        cd[str(Q)] = {"wall_ms_median": statistics.median(ts), "wall_ms_all": ts}
        print(f"cdist_cosine {n} x {Q}: {statistics.median(ts):.2f} ms wall", flush=True)
    result["cdist_cosine"] = {"rows": n, "timing": "host wall time around the blocking call (upload, float64 kernel, full matrix back)",
                              "Q": cd}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
