"""Seeded cases and the float64 restatement for the gallery search (csrc/gallery.hip; tests/test_gallery_host.py,
tests/test_gallery_gpu.py).  There is no reference counterpart for identification: this restatement is the oracle.

    rows, queries   normalised in float64 (in-order sum of squares, as the library's host code), the quotient rounded once to
                    fp32 — what `put` stores and what the scan multiplies
    score           the float64 dot product of those fp32 rows
    order           (score descending, slot ascending)

The bound B(dim) = (dim + 8) 2^-24 is derived, not measured: rounding the unit rows to fp32 moves a cosine by at most about
3 * 2^-24 (each operand's rounding contributes <= 2^-24 * sum |a_i b_i| <= 2^-24, plus the second-order term), and fp32
accumulation of `dim` products in any order moves it by <= gamma_dim * sum |a_i b_i| <= dim * 2^-24 * (1 + o(1)); the remaining
5 * 2^-24 cover the o(1).  1.57e-5 at dim 256.  The tests print the observed maximum next to it."""
import itertools

import numpy as np


def bound(dim: int) -> float:
    return (dim + 8) * 2.0 ** -24


def normalise(x: np.ndarray) -> np.ndarray:
    """float32 [n, dim] -> float32 [n, dim] unit rows as `put` stores them"""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    nrm = np.sqrt(np.cumsum(x64 * x64, axis=1)[:, -1])          # cumsum: the in-order sum
    return (x64 / nrm[:, None]).astype(np.float32)


def true_cosine(rows: np.ndarray, queries: np.ndarray) -> np.ndarray:
    """float64 [Q, n]: the cosine of the inputs as given, nothing rounded to fp32 on the way"""
    r, q = np.asarray(rows, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return q @ r.T


def ref_scores(rows: np.ndarray, queries: np.ndarray, valid=None) -> np.ndarray:
    """float64 [Q, n]: the restatement; -inf where valid[slot] is False"""
    s = normalise(queries).astype(np.float64) @ normalise(rows).astype(np.float64).T
    if valid is not None:
        s[:, ~np.asarray(valid, dtype=bool)] = -np.inf
    return s


def select(scores: np.ndarray, top_n: int):
    """scores [Q, n] (-inf = not a valid row) -> (scores [Q, top_n] in the dtype given, slots int64 [Q, top_n]) by
    (score descending, slot ascending); slot -1 / score -inf beyond the number of valid rows"""
    Q, n = scores.shape
    out_s = np.full((Q, top_n), -np.inf, dtype=scores.dtype)
    out_i = np.full((Q, top_n), -1, dtype=np.int64)
    for q in range(Q):
        ok = np.nonzero(scores[q] > -np.inf)[0]
        order = ok[np.lexsort((ok, -scores[q][ok].astype(np.float64)))][:top_n]
        out_s[q, :len(order)] = scores[q][order]
        out_i[q, :len(order)] = order
    return out_s, out_i


def gallery_case(seed: int, rows: int, Q: int, dim: int, scaled: bool = True):
    """(rows f32 [rows, dim], queries f32 [Q, dim]); with `scaled`, every third row / query is scaled by 1e-20 and the
    next by 1e+20 (normalisation makes the scale irrelevant)"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((rows, dim), dtype=np.float32)
    q = rng.standard_normal((Q, dim), dtype=np.float32)
    if scaled:
        for a in (r, q):
            a[1::3] *= np.float32(1e-20)
            a[2::3] *= np.float32(1e+20)
    return r, q


def planted_case(seed: int, rows: int, Q: int, dim: int, noise: float = 0.3):
    """queries = gallery rows + noise: (rows, queries, the planted slot of every query)"""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((rows, dim), dtype=np.float32)
    at = rng.choice(rows, size=Q, replace=False)
    q = r[at] + np.float32(noise) * rng.standard_normal((Q, dim), dtype=np.float32)
    return r, q, at


def assignment_case(seed: int, K: int, n_cand: int):
    """dense candidate lists for assign_identities: scores [K, n_cand] in (0, 1), slots [K, n_cand] (every label lists every
    candidate slot, in score order)"""
    rng = np.random.default_rng(seed)
    dense = rng.uniform(0.05, 0.95, size=(K, n_cand))
    ids = np.sort(rng.choice(1000, size=n_cand, replace=False))
    order = np.argsort(-dense, axis=1, kind="stable")
    return np.take_along_axis(dense, order, axis=1), ids[order]


def brute_force_objective(scores: np.ndarray, slots: np.ndarray, threshold: float) -> float:
    """max over all partial one-to-one matchings of sum (score - threshold) over matched pairs with score >= threshold"""
    K = scores.shape[0]
    cands = sorted({int(s) for s in slots.ravel() if s >= 0})
    val = {(k, int(s)): float(v) for k in range(K) for s, v in zip(slots[k], scores[k]) if s >= 0}
    best = 0.0
    for choice in itertools.product([None] + cands, repeat=K):
        used = [c for c in choice if c is not None]
        if len(used) != len(set(used)):
            continue
        total, ok = 0.0, True
        for k, c in enumerate(choice):
            if c is None:
                continue
            v = val.get((k, c))
            if v is None or v < threshold:
                ok = False
                break
            total += v - threshold
        if ok:
            best = max(best, total)
    return best


def objective(scores: np.ndarray, slots: np.ndarray, threshold: float, matched) -> float:
    total = 0.0
    for k, m in enumerate(matched):
        if m is None:
            continue
        j = np.nonzero(slots[k] == m)[0]
        assert len(j) >= 1 and scores[k][j[0]] >= threshold           # only listed candidates at or above the threshold
        total += float(scores[k][j[0]]) - threshold
    return total
