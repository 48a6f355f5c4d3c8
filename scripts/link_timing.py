#!/usr/bin/env python
"""Time ops.link_speakers (csrc/linkage.hip, dzn_link_speakers) on one device against the scipy definition.

    python scripts/link_timing.py [--out profiles/link_timing.json] [--rows 64,128,...] [--scipy-max 8192]

Per row count: a seeded planted-people corpus (dim 256, recordings of 4-8 labels, noise 0.5, threshold 0.5); the whole
ops.link_speakers call by the host clock around the synchronising call (median of 5 after a warm-up); merges, step launches
and row rescans from the step descriptor (dzn_link_speakers_last); the distance kernel alone by HIP events; scipy's
pdist + mask + linkage("complete") + count for the same input up to --scipy-max rows, and whether both gave the same number of
merges.  The "auto" crossover of linking.SpeakerLinker (linking.HIP_LINK_MIN) is read off this table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def corpus(n: int, dim: int = 256, seed: int = 0, noise: float = 0.5):
    """n voiceprints in recordings of 4-8 labels; a recording's labels are distinct people out of max(8, n // 16)"""
    r = np.random.default_rng(seed)
    people = r.standard_normal((max(8, n // 16), dim))
    rows, group = [], []
    g = 0
    while len(rows) < n:
        k = min(int(r.integers(4, 9)), n - len(rows))
        who = r.choice(len(people), size=k, replace=False)
        rows.extend(people[who] + noise * r.standard_normal((k, dim)))
        group.extend([g] * k)
        g += 1
    return np.asarray(rows, dtype=np.float32), np.asarray(group, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/link_timing.json")
    ap.add_argument("--rows", default="64,128,256,512,1024,8192,32768")
    ap.add_argument("--scipy-max", type=int, default=8192)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from diarizen_amd import linking, ops
    table = []
    for n in [int(v) for v in a.rows.split(",")]:
        emb, group = corpus(n)
        ops.link_speakers(emb, group, a.threshold)                      # warm-up (arena, code objects)
        times, pd = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            Z, m = ops.link_speakers(emb, group, a.threshold)
            times.append(time.perf_counter() - t)
            last = ops.link_speakers_last()
            pd.append(last["pdist_ms"])
        row = {"n": n, "dim": int(emb.shape[1]), "recordings": int(group.max()) + 1, "threshold": a.threshold, "merges": m,
               "device_ms": round(1e3 * statistics.median(times), 3), "device_ms_all": [round(1e3 * t, 3) for t in times],
               "pdist_kernel_ms": round(statistics.median(pd), 3), "launches": last["launches"], "rescans": last["rescans"],
               "useful_launches_per_merge": round((m + last["rescans"]) / max(m, 1), 4)}
        if n <= a.scipy_max:
            st = []
            for _ in range(3 if n <= 1024 else 1):
                t = time.perf_counter()
                Zs, ms = linking.link_scipy(emb, group, a.threshold)
                st.append(time.perf_counter() - t)
            row["scipy_ms"] = round(1e3 * statistics.median(st), 3)
            row["scipy_merges"] = ms
            row["same_prefix_ids"] = bool(ms == m and np.array_equal(Zs[:m][:, [0, 1, 3]], Z[:, [0, 1, 3]]))
            row["worst_height_deviation"] = float(np.abs(Zs[:m, 2] - Z[:, 2]).max()) if m and ms == m else None
        else:
            row["scipy_ms"] = None                                      # not run: beyond --scipy-max
        print(json.dumps(row), flush=True)
        table.append(row)
    out = {"device": torch.cuda.get_device_name(0), "what": "ops.link_speakers, host clock around the blocking call, median of "
           f"{a.reps} after a warm-up; scipy = pdist + mask + linkage(complete)", "table": table}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
