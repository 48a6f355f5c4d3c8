"""Shared inputs and references of the speaker-linking tests (tests/test_linking_host.py, tests/test_linking_gpu.py): seeded
planted-people corpora, the group layouts, the scipy definition, the distance bound and the input condition under which a
device dendrogram can be compared with scipy's row by row."""
import functools

import numpy as np

BIG = 4.0

# row counts at the 64-row tile and the 256-row workgroup edges; dims: one k-tile, not a multiple of 16, the pipeline's
ROWS = (2, 3, 63, 64, 65, 255, 256, 257, 513)
DIMS = (16, 20, 256)
LAYOUTS = ("singletons", "one_group", "groups_3_4", "huge_plus_singletons")
SEED = 1      # of every case; a case that fails `input_condition` gets another seed in SEEDS, never another factor
SEEDS = {}


def distance_bound(dim: int) -> float:
    """|device distance - scipy distance| <= 2 (dim + 8) 2^-53 for ANY summation order: float32 x float32 products are exact in
    float64, so each side's dot product and norms carry only the (dim - 1) roundings of the sums, the two square roots, the
    product of the norms, the quotient and the subtraction from 1 — every one at most 2^-53 relative on values <= 1 after the
    division: each side's cosine is within (dim + 8) units of 2^-53 of the true one."""
    return 2.0 * (dim + 8) * 2.0 ** -53


def planted(n: int, dim: int, seed: int, noise: float = 0.5) -> np.ndarray:
    """n float32 voiceprints of max(1, n // 6) planted people: a person's direction plus isotropic noise"""
    r = np.random.default_rng(seed)
    people = r.standard_normal((max(1, n // 6), dim))
    who = r.integers(0, len(people), n)
    return (people[who] + noise * r.standard_normal((n, dim))).astype(np.float32)


def groups(layout: str, n: int) -> np.ndarray:
    if layout == "singletons":             # plain complete linkage
        return np.arange(n, dtype=np.int32)
    if layout == "one_group":              # nothing may merge
        return np.zeros(n, dtype=np.int32)
    if layout == "groups_3_4":             # sizes 3, 4, 3, 4, ...: rows 255 .. 258 are one group (252 = 36 * 7)
        g, out = 0, []
        while len(out) < n:
            out += [g] * (3 if g % 2 == 0 else 4)
            g += 1
        return np.array(out[:n], dtype=np.int32)
    if layout == "huge_plus_singletons":   # the first half is one recording, the rest one row each
        g = np.arange(n, dtype=np.int32) + 1
        g[:max(1, n // 2)] = 0
        return g
    raise ValueError(layout)


def definition(emb: np.ndarray, group: np.ndarray):
    """-> (the complete-linkage dendrogram of the masked cosine distances, the sorted ALLOWED distances)"""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    y = pdist(emb.astype(np.float64), "cosine")
    i, j = np.triu_indices(len(emb), 1)
    same = group[i] == group[j]
    allowed = np.sort(y[~same])
    y[same] = BIG
    return linkage(y, "complete"), allowed


def thresholds(allowed: np.ndarray) -> list:
    """below the smallest allowed distance, inside the distribution (midway between two neighbours at the 30 % quantile), 2.0"""
    if len(allowed) == 0:
        return [1.0, 2.0]
    k = min(int(0.3 * len(allowed)), len(allowed) - 2)
    inside = 0.5 * (allowed[k] + allowed[k + 1]) if len(allowed) >= 2 else 1.5 * allowed[0]
    return [0.5 * allowed[0], float(inside), 2.0]


def input_condition(allowed: np.ndarray, ts, dim: int) -> float:
    """the smallest of: the gaps between allowed distances, their distances to every threshold — in units of the bound.  A
    comparison with scipy row by row needs this to be >= 50: then neither side's rounding can reorder two merges or move one
    across a threshold."""
    b = distance_bound(dim)
    worst = np.inf
    if len(allowed) >= 2:
        worst = min(worst, np.diff(allowed).min() / b)
    for t in ts:
        if len(allowed):
            worst = min(worst, np.abs(allowed - t).min() / b)
    return worst


@functools.lru_cache(maxsize=None)
def case(n: int, dim: int, layout: str):
    """-> (emb f32 [n, dim], group i32 [n], Z of the definition, thresholds), computed once per session and read-only"""
    emb = planted(n, dim, SEEDS.get((n, dim, layout), SEED))
    group = groups(layout, n)
    Z, allowed = definition(emb, group)
    ts = thresholds(allowed)
    assert input_condition(allowed, ts, dim) >= 50.0, (n, dim, layout)
    for a in (emb, group, Z):
        a.setflags(write=False)
    return emb, group, Z, ts


def linker_for(emb, group, threshold, backend, dim):
    """a SpeakerLinker with one `add` per group, in order of first appearance -> (linker, {row: (recording, label)})"""
    from diarizen_amd.linking import SpeakerLinker
    L = SpeakerLinker(threshold, dim=dim, backend=backend)
    key = {}
    for g in dict.fromkeys(group.tolist()):
        rows = np.flatnonzero(group == g)
        L.add(f"rec{g}", emb[rows])
        for k, r in enumerate(rows):
            key[int(r)] = (f"rec{g}", k)
    return L, key


def cannot_link_holds(links) -> bool:
    """no identity holds two labels of one recording"""
    seen = set()
    for (rec, _), i in links.identity.items():
        if (rec, i) in seen:
            return False
        seen.add((rec, i))
    return True
