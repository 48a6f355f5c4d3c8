"""Shared by test_live_scores_host.py and test_live_scores_gpu.py: the aggregation cases of tests/golden/scores_ref.npz
(reference-made, scripts/gen_scores_golden.py) with their window start frames, and the partitions of [0, T) a range call is cut
at.  numpy only; nothing here touches a device."""
from __future__ import annotations

import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "scores_ref.npz"))
AGG = [str(c) for c in G["agg_cases"]]


def case(name):
    """-> dict: soft f32 [C, L, S], hard int8 [C, S], starts int32 [C], duration, warm_up, K = the golden's columns, T = the
    golden's rows (cropped where the reference cropped), full = every frame the windows cover, ref = the golden scores"""
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import _frame_grid, receptive_field
    dur, ratio, _, w0, w1 = (float(v) for v in G[f"{name}_args"])
    soft, hard, ref = G[f"{name}_soft"], G[f"{name}_hard"].astype(np.int8), G[f"{name}_scores"]
    chunks = SlidingWindow(start=0.0, duration=dur, step=ratio * dur)
    _, starts, full = _frame_grid(soft.shape[0], soft.shape[1], chunks, receptive_field())
    return dict(soft=soft, hard=hard, starts=starts, duration=dur, warm_up=(w0, w1), K=ref.shape[1], T=len(ref), full=full,
                ref=ref, chunks=chunks)


def partitions(d):
    """cuts of [0, T): none; at every window's start frame and at start + L; one-frame ranges (and an empty one) around the
    first window's end"""
    T, L = d["T"], d["soft"].shape[1]
    at = sorted({int(s) + o for s in d["starts"] for o in (0, L)} & set(range(1, T)))
    mid = min(L, T - 1)
    ones = sorted({t for t in (mid - 1, mid, mid, mid + 1, T - 1) if 0 < t < T} | ({mid} if 0 < mid < T else set()))
    return {"whole": [], "window_edges": at, "single_frames": ones + ([mid] if 0 < mid < T else [])}


def bounds(T, cuts):
    b = [0] + sorted(int(c) for c in cuts) + [T]
    return list(zip(b[:-1], b[1:]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
