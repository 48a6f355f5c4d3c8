"""Shared inputs and references of the speaker-registry tests (tests/test_registry_host.py, tests/test_registry_gpu.py): seeded
stored sets with their identities, a new recording, the float64 table of max distances, the scipy node-matrix definition of
the assignment and the input condition under which a device table can decide exactly what the reference decides."""
import functools

import numpy as np

from _linking_cases import BIG, distance_bound, planted, thresholds

# stored rows at the 64-entry chunk edges and past several chunks; dims: one staging block, not a multiple of 16, the pipeline's;
# new rows: one, two, and the edges of the 32-query group (the sweep's widest form; a 33rd query opens a second group)
STORED = (1, 2, 63, 64, 65, 255, 256, 257, 513)
DIMS = (16, 20, 256)
NEW = (1, 2, 31, 32, 33)
SEED = 1      # of every case; a case that fails the input condition gets another seed in SEEDS, never another factor
SEEDS = {}

# the GPU tests run the whole product, and the edges of the narrower forms of the sweep (8 and 16 queries wide: K = 8 | 9 and
# 16 | 17; 40 = 32 + 8 queries: a full group and a narrow one) where the member index has identities that span chunks
GROUP_EDGES = (8, 9, 16, 17, 40)
GPU_CASES = [(n, dim, k) for n in STORED for dim in DIMS for k in NEW] + \
            [(n, dim, k) for n, dim in ((65, 20), (513, 256)) for k in GROUP_EDGES]


def stored_identities(n: int) -> np.ndarray:
    """identity numbers of n stored rows: identity 0 holds a third of all rows (interleaved with the others, so its members
    are scattered over the storage), then identities of 65, 64, 63 and 2 members as far as the rows reach, singletons for the
    rest; number 1 is skipped (an identity without a stored row), and the numbers are not in storage order"""
    ident = np.full(n, -1, dtype=np.int32)
    ident[::3] = 0
    free = np.flatnonzero(ident < 0)
    nxt, at = 2, 0
    for size in (65, 64, 63, 2):
        if at + size <= len(free):
            ident[free[at:at + size]] = nxt
            nxt += 1
            at += size
    rest = free[at:]
    ident[rest] = nxt + np.arange(len(rest))[::-1]          # singletons, numbered against the storage order
    return ident


def table(queries: np.ndarray, rows: np.ndarray, ident: np.ndarray, width: int) -> np.ndarray:
    """float64 [K, width]: per identity number the max over its rows of scipy's cosine distance; +inf where it holds none"""
    from scipy.spatial.distance import cdist
    d = cdist(queries.astype(np.float64), rows.astype(np.float64), "cosine")
    out = np.full((len(queries), width), np.inf)
    for i in np.unique(ident):
        out[:, i] = d[:, ident == i].max(axis=1)
    return out


def definition(D: np.ndarray, threshold: float) -> dict:
    """the scipy node-matrix definition: D float64 [K, C] over the C NON-EMPTY identities -> {k: column}"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    K, C = D.shape
    if K + C < 2:
        return {}
    M = np.full((C + K, C + K), BIG)
    M[:C, C:] = D.T
    M[C:, :C] = D
    np.fill_diagonal(M, 0.0)
    flat = fcluster(linkage(squareform(M, checks=False), "complete"), threshold, "distance")
    out = {}
    for k in range(K):
        same = np.flatnonzero(flat[:C] == flat[C + k])
        assert len(same) <= 1
        if len(same):
            out[k] = int(same[0])
    return out


def greedy(D: np.ndarray, threshold: float) -> dict:
    """the greedy rule on the reference table, written independently of diarizen_amd.registry.greedy_assign"""
    D = np.array(D, copy=True)
    out = {}
    while D.size and np.isfinite(D).any():
        k, c = np.unravel_index(np.argmin(D), D.shape)
        if D[k, c] > threshold:
            break
        out[int(k)] = int(c)
        D[k, :] = np.inf
        D[:, c] = np.inf
    return out


def input_condition(D: np.ndarray, ts, dim: int) -> float:
    """the smallest of: the gaps between the entries of D, their distances to every threshold — in units of the bound"""
    b = distance_bound(dim)
    v = np.sort(D.ravel())
    worst = np.inf
    if len(v) >= 2:
        worst = min(worst, np.diff(v).min() / b)
    for t in ts:
        worst = min(worst, np.abs(v - t).min() / b)
    return worst


@functools.lru_cache(maxsize=None)
def case(n: int, dim: int, K: int):
    """-> (stored f32 [n, dim], ident i32 [n], queries f32 [K, dim], D float64 [K, I] (+inf at empty numbers), thresholds),
    computed once per session and read-only; asserts the input condition on the reference alone"""
    emb = planted(n + K, dim, SEEDS.get((n, dim, K), SEED))
    stored, queries = emb[:n], emb[n:]
    ident = stored_identities(n)
    D = table(queries, stored, ident, int(ident.max()) + 1)
    finite = D[:, np.isfinite(D[0])]
    ts = thresholds(np.sort(finite.ravel()))
    assert input_condition(finite, ts, dim) >= 50.0, (n, dim, K)
    for a in (stored, ident, queries, D):
        a.setflags(write=False)
    return stored, ident, queries, D, ts


def columns(D: np.ndarray) -> np.ndarray:
    """the identity numbers that hold a row"""
    return np.flatnonzero(np.isfinite(D[0]))


def assignment(D: np.ndarray, threshold: float) -> dict:
    """{k: identity number} by the scipy definition"""
    cols = columns(D)
    return {k: int(cols[c]) for k, c in definition(D[:, cols], threshold).items()}


def seeded_registry(stored, ident, threshold, backend, dim, capacity=None):
    """a SpeakerRegistry that holds `stored` under `ident`: built through SpeakerLinker / from_links with one recording per
    stored row (rows of one identity are different recordings), identities renumbered by the links -> (registry, {number in
    `ident`: identity in the registry})"""
    from diarizen_amd.linking import SpeakerLinker, SpeakerLinks
    from diarizen_amd.registry import SpeakerRegistry
    L = SpeakerLinker(threshold, dim=dim, backend="scipy")
    for r in range(len(stored)):
        L.add(f"rec{r}", stored[r:r + 1])
    number = {}
    for i in ident.tolist():
        number.setdefault(i, len(number))
    keys = [(f"rec{r}", 0) for r in range(len(stored))]
    ids = [number[i] for i in ident.tolist()]
    links = SpeakerLinks(keys, ids, {i: 0.0 for i in number.values()}, [], threshold, "scipy")
    reg = SpeakerRegistry.from_links(L, links, capacity=capacity or len(stored) + 64, backend=backend)
    return reg, number
