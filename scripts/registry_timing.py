#!/usr/bin/env python
"""Time one `add` of a recording into a speaker registry (csrc/registry.hip, diarizen_amd/registry.py) on one device.

    python scripts/registry_timing.py [--out profiles/registry_timing.json] [--rows 64,...,1000000] [--batch-max 190000]

Per number N of stored rows: a seeded planted-people corpus (dim 256, people of about 8 voiceprints each, noise 0.5, threshold
0.5) stored under the planted people as identities, and a recording of K = 8 new voiceprints.  Recorded, each the median of
--reps after a warm-up, by the host clock around the blocking calls unless stated:
  hip     match_ms     ops.Registry.match with a current member index: upload of the queries, sweep, reduce, download of triples
          kernel_ms    the launches of that call alone, by HIP events; stored bytes / kernel_ms = the sweep's rate
          add_ms       append of the K rows + the first match after it: what an add costs, index rebuild and upload included
  numpy   registry.cosine_table + greedy_assign on the same input: the "numpy" backend's share of an add
  batch   SpeakerLinker(backend="hip").link() over the N + K rows as one recording per 8 rows, up to --batch-max rows: the
          whole-corpus re-link an add would cost without a registry (8 n^2 bytes of arena).  The sizes between 10^5 and
          2 * 10^5 look for the largest corpus the batch path still links; after the first size that fails no larger one is tried
and whether the device's triples are the numpy backend's.  The "auto" crossover of registry.SpeakerRegistry
(registry.REGISTRY_HIP_MIN) is read off this table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def corpus(n: int, k: int, dim: int = 256, seed: int = 0, noise: float = 0.5):
    """n stored voiceprints of max(8, n // 8) people + k new ones of distinct people -> (stored, identity per row, new)"""
    r = np.random.default_rng(seed)
    people = r.standard_normal((max(8, n // 8), dim)).astype(np.float32)
    who = r.integers(0, len(people), n).astype(np.int32)
    stored = people[who]
    for a in range(0, n, 65536):
        stored[a:a + 65536] += noise * r.standard_normal((len(stored[a:a + 65536]), dim)).astype(np.float32)
    new = people[r.choice(len(people), size=k, replace=False)] + noise * r.standard_normal((k, dim)).astype(np.float32)
    return stored, who, new.astype(np.float32)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return round(statistics.median(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/registry_timing.json")
    ap.add_argument("--rows", default="64,256,1000,10000,100000,150000,170000,185000,1000000")
    ap.add_argument("--batch-max", type=int, default=190000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from diarizen_amd import ops, registry
    from diarizen_amd.linking import SpeakerLinker
    table = []
    batch_failed = False
    for n in [int(v) for v in a.rows.split(",")]:
        stored, who, new = corpus(n, a.k)
        dim = stored.shape[1]
        row = {"n": n, "dim": dim, "k": a.k, "identities": int(len(np.unique(who))), "threshold": a.threshold}
        reg = ops.Registry(dim, n + (a.reps + 2) * a.k)
        try:
            reg.append(stored, who)
            got = reg.match(new, a.threshold)
            kern = []

            def match():
                reg.match(new, a.threshold)
                kern.append(reg.last_launch_ms())

            row["hip_match_ms"] = median_ms(match, a.reps)
            row["hip_kernel_ms"] = round(statistics.median(kern[1:]), 4)
            row["stored_gb"] = round(n * dim * 4 / 1e9, 4)
            row["kernel_tb_per_s"] = round(n * dim * 4 / 1e12 / (row["hip_kernel_ms"] / 1e3), 3)
            fresh = iter(range(int(who.max()) + 1, int(who.max()) + 1 + (a.reps + 2) * a.k))

            def add():      # the K rows under new identities, then the match that rebuilds the index
                reg.append(new, np.array([next(fresh) for _ in range(a.k)], dtype=np.int32))
                reg.match(new, a.threshold)

            row["hip_add_ms"] = median_ms(add, a.reps)
        finally:
            reg.close()

        def host():
            cols, D = registry.cosine_table(new, stored, who)
            kk, cc = np.nonzero(D <= a.threshold)
            return kk, cols[cc], D[kk, cc]

        ref = host()
        row["numpy_ms"] = median_ms(lambda: registry.greedy_assign(*host(), a.threshold), min(a.reps, 3))
        row["same_entries"] = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
        row["entries"] = int(len(ref[0]))
        row["batch_ms"] = None
        if n + a.k <= a.batch_max and not batch_failed:
            L = SpeakerLinker(a.threshold, dim=dim, backend="hip")
            rows = np.concatenate([stored, new])
            for j, r0 in enumerate(range(0, len(rows), 8)):
                L.add(j, rows[r0:r0 + 8])
            try:
                row["batch_ms"] = median_ms(L.link, 1)
                row["batch_matrix_gb"] = round(8 * len(rows) ** 2 / 1e9, 2)
            except (MemoryError, RuntimeError) as e:
                row["batch_error"] = type(e).__name__
                batch_failed = True
            ops._lib.load().dzn_host_workspace_release(-1)
        print(json.dumps(row), flush=True)
        table.append(row)
    out = {"device": torch.cuda.get_device_name(0),
           "what": "one add of K new voiceprints into a registry of n stored rows; host clock around the blocking calls, median "
                   "after a warm-up; kernel_ms by HIP events; batch = SpeakerLinker(hip).link() over the n + K rows",
           "table": table}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
