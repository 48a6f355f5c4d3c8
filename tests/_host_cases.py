"""Shared by test_host_kernels_gpu.py (device) and test_host_kernels_host.py (CPU): case tables, seeded inputs, references, mutants
and bounds of the device kernels of the HOST stage — csrc/linkage.hip (pdist_kernel + the step loop through dzn_linkage_centroid,
row_norm_* + cdist_cosine_kernel through dzn_cdist_cosine), csrc/vbx.hip (vb_setup, vb_accum, vb_reduce, vb_estep through
ops.VbxState) and the integer / byte kernels of csrc/post.hip (prepare_masks, count_accum / count_finalize, cluster_accum,
hysteresis_kernel at its block edge).  numpy / scipy only; nothing here touches a device.

Every family has ONE `<k>_run(case, inp, ..., mutant)` that states the operation (with the exact sum it is the reference, with a
sequential float64 sum an IDEAL kernel, with `mutant` one of the subtly wrong kernels test_host_kernels_host.py holds the checks
against) and one `<k>_bound(case, inp, s)`, DERIVED, never tuned.  These kernels compute in float64: u = 2^-53, n counts TERMS.

  sums            n float64 terms t_i added in ANY order: (n + 8) u sum|t_i| (as _small_cases.py counts an accumulation; a fused
                  multiply-add only removes roundings).  This is the ACCUMULATION share; every bound takes a factor `s` on it and
                  the host test shows that an ideal float64 kernel stays inside at s = 1/4.  Single roundings enter at face value.
  sqrt, division  1 ulp = 2 u each (nothing here relies on the device's double sqrt / division being correctly rounded).
  exp, log        2 ulp = 4 u relative (ULP_FN), as in _small_cases.py.
  references      sums in np.longdouble (64-bit mantissa: 2^-11 u per operation) or math.fsum.

linkage    Z against scipy.cluster.hierarchy.linkage(e.astype(float64), "centroid"): ids and sizes exactly, every height within the
           project's 1e-12 max(1, max height), a second call the same bits.  A merge of two SINGLETONS is a pure pdist_kernel output
           sqrt(sum_k (a_k - b_k)^2): a_k - b_k is one rounding (u, relative, so 2 u on the square), the square another (u), the
           dim squares are all >= 0 so sum|t| is the sum: (dim + 8) u + 3 u relative on the sum, HALVED by the square root, + 2 u for
           the square root itself: (dim + 8) s u / 2 + 1.5 u + 2 u <= (dim + 8 + 2) u with s <= 1 — the bound used, relative to the
           longdouble value (scipy's own pdist carries the same kind of error, so it is not the reference for this check).
           The ids only mean something where scipy's own dendrogram is stable: test_host_kernels_host.py perturbs the condensed
           distances by relative 1e-12 (3 seeds) and asks for unchanged ids on every case; LK_SEED holds the seeds chosen for that on
           the CPU when the table was written.  The G > 256 branch of step2_kernel needs n > 65 536 rows (a 34 GB matrix): out of a
           test's reach, left to tests/test_ops_gpu.py's 30 k golden, which does not reach it either.
cdist      the kernel's own statement in float64, in order (seq_sum): p = e_i v_i, s = s + p; norms sqrt of the in-order square sum;
           cos = s / (|e| |v|), clipped to [-1, 1]; 1 - cos.  Products, sums and the product of the norms are IEEE and in the same
           order on both sides, so only the two square roots and the division can differ: 3 x 2 u = 6 u relative on cos, 8 u with the
           second-order terms; the last subtraction rounds what it is given: |d out| <= 8 u |cos| + u.  EXACT: the NaN pattern, equal
           bits for identical rows, and 0 <= out <= 2 (what the clip is for: without it a row that IS a centroid gives -2 u, inside
           the numeric bound).  Against the longdouble dot product the in-order emulation itself stays inside
           s (dim + 8) u sum|e v| / den + 8 u |cos| before the clip (the single roundings of the two square roots and the division at face value —
           at dim = 3 a quarter of (dim + 8) u is 2.75 u, less than those roundings alone, and the bare first term is missed by 1.45;
           the norms' own accumulation is relative to a sum of squares, i.e. without cancellation, and is counted in the first term
           since sum|e v| / den >= |cos|).
vbx        rho = X sqrt(Phi): sqrt 2 u, product u -> 3 u |rho|.  stats: Fs[k, d] = sum_e gamma rho: (E + 8) s u sum|gamma rho| +
           3 u sum|gamma rho| (+ u per product, inside the +8); Ns[k]: (E + 8) s u sum gamma.
           G = -0.5 (sum x^2 + D log 2 pi): dG = 0.5 ((D + 8) s u sum x^2 + u D log 2 pi) + 2 u |G|.
           a[k] = Fa (dot - ck + G) + lpi with dot = sum_d rho alpha: da = Fa ((D + 8) s u S + 3 u S + dG + u |dot - ck| +
           u |dot - ck + G|) + u |a - lpi| + u |a|, S = sum|rho alpha|.
           logsumexp is 1-Lipschitz in the sup norm of a: dl = max_k da + ((K + 8) s u + 4 u) [the sum of K exponentials >= 1 and
           its four single roundings: a - amax weighted by exp(a - amax) <= 1/e, twice, the log's argument, the shift] + 4 u
           [exp] + 4 u |log se| [log] + u |l|.  gamma = exp(a - l): relative expm1(da + dl + u |a - l| + 4 u) — the rounding of the
           difference a - l is u |a - l|, which matters for the far tails (|a - l| up to 745) — + 2^-1072 for the
           denormal range.  total = sum_e l: (E + 8) s u sum|l| + sum dl.  Rows of gamma sum to 1 within (K + 8) u + sum_k bound.
           Where one speaker leads by more than 745 the others' exp underflows: gamma is EXACTLY 0 / 1 there, never NaN.
post       integers and bytes: exact equality.  prepare_masks against scipy.ndimage.median_filter(size=(1, median, 1),
           mode="reflect") — 'reflect' has period 2L, also for windows longer than the signal — and the numpy mask expression of
           tests/test_emb_gpu.py.  ONE pair of the axes is not in the table: L = 2 with median = 21.  scipy's offset table
           (ni_support.c, NI_InitFilterOffsets) folds a tap below -2L by a multiple of 2L and then reflects a result of exactly 0 to
           index -1, one element BEFORE the line; the only tap of these axes that lands there is t - 10 = -8 = -4L at L = 2, so
           there scipy's output depends on whatever precedes the window in memory and is no reference.  speaker_count / cluster_activations against np.add.at with np.rint in float32 (half to even);
           hysteresis against postprocess._hysteresis on scores that are exactly 0, 0.5 or 1.
"""
from __future__ import annotations

import math

import numpy as np

from _small_cases import phase_sum, seq_sum, worst_ratio          # noqa: F401  (re-exported for the two test files)

U = 2.0 ** -53
ULP_FN = 4 * U
F32, F64, LD = np.float32, np.float64, np.longdouble
LOG_2PI = 1.8378770664093453            # the constant of vb_setup_kernel and of np.log(2 * np.pi)


def exact_sum(x, axis):
    return np.sum(x.astype(LD), axis=axis)


def chunk_sum(n):
    """rows in chunks of n, in order inside a chunk, then the chunks in order (vb_accum_kernel + vb_reduce_kernel)"""
    def f(x, axis):
        x = np.moveaxis(x, axis, 0)
        parts = [seq_sum(x[i:i + n], 0) for i in range(0, x.shape[0], n)]
        return seq_sum(np.stack(parts), 0)
    return f


def _seed(name, i):
    return np.random.default_rng([sum(map(ord, name)), i])


# ---- linkage + pdist ------------------------------------------------------------------------------------------------------
LK_N = (2, 3, 63, 64, 65, 129, 257)
LK_DIM = (1, 3, 15, 16, 17, 33, 256)
LK_SCALE = (1e-3, 1.0, 1e3)
LK_EXTRA = ((129, 256), (64, 17), (65, 15), (257, 17))
LK_SEED = {}                            # (n, dim) -> the seed that replaced n + dim because scipy's ids were not stable with it
LK_TOL = 1e-12


def lk_cases():
    pairs = [(n, LK_DIM[(i + 2 * j) % 7]) for i, n in enumerate(LK_N) for j in range(3)] + list(LK_EXTRA)
    out = [dict(i=i, kind="clustered", n=n, dim=dim, scale=LK_SCALE[i % 3], seed=LK_SEED.get((n, dim), n + dim))
           for i, (n, dim) in enumerate(pairs)]
    out.append(dict(i=len(out), kind="triplets", n=129, dim=17, scale=1.0, seed=5))
    out.append(dict(i=len(out), kind="inversions", n=65, dim=3, scale=1.0, seed=7))
    return out


def lk_inputs(c):
    """clustered: oracle.gen_golden.linkage_scale_case's recipe (elementwise float32 operations on seeded draws) with the case's
    n, dim and scale; triplets: 40 tight triplets (two members closer to each other than to the third) + 9 loose points, shuffled
    over the tiles; inversions: unstructured points in 3 dimensions"""
    r = np.random.default_rng(c["seed"])
    n, dim = c["n"], c["dim"]
    if c["kind"] == "clustered":
        cent = r.standard_normal((4, dim), dtype=F32)
        lab = r.integers(0, 4, n)
        noise = r.standard_normal((n, dim), dtype=F32)
        e = (cent[lab] * F32(0.25) + noise * F32(0.11)) * F32(c["scale"])
    elif c["kind"] == "triplets":
        centre = r.standard_normal((40, dim))
        v, w = r.standard_normal((40, dim)), r.standard_normal((40, dim))
        tri = np.stack([centre + 3e-4 * v, centre - 3e-4 * v, centre + 1e-3 * w], 1).reshape(120, dim)
        e = np.concatenate([tri, r.standard_normal((n - 120, dim))])[r.permutation(n)]
    else:
        e = r.standard_normal((n, dim))
    return dict(e=np.ascontiguousarray(e, dtype=F32))


def lk_ref(c, inp):
    """scipy's dendrogram + the longdouble distance of every singleton-singleton merge (NaN elsewhere)"""
    from scipy.cluster.hierarchy import linkage
    e = inp["e"].astype(F64)
    Z = linkage(e, "centroid")
    single = (Z[:, 0] < c["n"]) & (Z[:, 1] < c["n"])
    d = np.full(len(Z), np.nan)
    a, b = e[Z[single, 0].astype(int)].astype(LD), e[Z[single, 1].astype(int)].astype(LD)
    d[single] = np.sqrt(((a - b) ** 2).sum(1)).astype(F64)
    return dict(Z=Z, single=single, pd=d)


def lk_pdist_model(e, mutant=None):
    """pdist_kernel in numpy: the full matrix [n, n], float64 squares added in the order of the columns"""
    n, dim = e.shape
    kd = 16 * (dim // 16) if mutant == "k_tail" else dim
    x = e.astype(F64)
    rows = np.arange(n)

    def block(src_j):
        acc = np.zeros((n, n))
        for k in range(kd):
            d = x[:, None, k] - src_j[None, :, k]
            acc = acc + d * d
        return np.sqrt(acc)
    D = block(x)
    if mutant == "j_tile":              # rows >= 64 of the j-tile come from the i-tile: D[i][j] uses row 64 bi + j % 64 for bj > bi
        bi, bj = rows[:, None] // 64, rows[None, :] // 64
        src = 64 * bi + rows[None, :] % 64
        ok = src < n
        xs = np.where(ok[..., None], x[np.minimum(src, n - 1)], 0.0)
        wrong = np.sqrt(((x[:, None, :kd] - xs[..., :kd]) ** 2).sum(2))
        up = bj > bi
        D = np.where(up, wrong, D)
        D = np.where(up.T, D.T, D)
    np.fill_diagonal(D, 0.0 if mutant == "diag_zero" else np.inf)
    return D


def lk_naive(D):
    """the greedy algorithm on a FULL matrix whose diagonal takes part (as the device's rows see it): the closest active pair,
    scipy's centroid update; stops at a row merged with itself"""
    n = len(D)
    D = D.copy()
    size, cid, act, Z = np.ones(n, int), np.arange(n), np.ones(n, bool), []
    for k in range(n - 1):
        M = np.where(act[:, None] & act[None, :], D, np.inf)
        x, y = divmod(int(np.argmin(M)), n)
        d = M[x, y]
        if x == y:
            Z.append((cid[x], cid[x], d, size[x]))
            break
        lo, hi = min(x, y), max(x, y)
        nlo, nhi = int(size[lo]), int(size[hi])
        Z.append((min(cid[lo], cid[hi]), max(cid[lo], cid[hi]), d, nlo + nhi))
        for z in np.nonzero(act)[0]:
            if z != lo and z != hi:
                dxi, dyi = D[lo, z], D[hi, z]
                D[hi, z] = D[z, hi] = math.sqrt((((nlo * dxi * dxi) + (nhi * dyi * dyi)) - (nlo * nhi * d * d) / (nlo + nhi)) / (nlo + nhi))
        act[lo], size[hi], cid[hi] = False, nlo + nhi, n + k
    return np.array(Z, dtype=F64)


def lk_model_Z(c, inp, mutant=None):
    """the dendrogram the numpy model of pdist_kernel leads to"""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    D = lk_pdist_model(inp["e"], mutant)
    if mutant == "diag_zero":
        return lk_naive(D)
    np.fill_diagonal(D, 0.0)
    return linkage(squareform(D, checks=False), "centroid")


def lk_same_ids(Z, ref):
    return Z.shape == ref.shape and np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]])


def lk_stable(c, inp, seeds=(0, 1, 2)):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    d = pdist(inp["e"].astype(F64))
    Z = linkage(d, "centroid")
    return all(lk_same_ids(linkage(d * (1 + 1e-12 * np.random.default_rng(s).uniform(-1, 1, d.shape)), "centroid"), Z) for s in seeds)


def lk_check(c, ref, Z):
    """(worst |height - scipy| / tolerance, worst singleton-merge error / bound); inf where ids or sizes differ"""
    if not lk_same_ids(Z, ref["Z"]):
        return math.inf, math.inf
    h = ref["Z"][:, 2]
    r1 = float(np.abs(Z[:, 2] - h).max() / (LK_TOL * max(1.0, h.max())))
    s = ref["single"]
    r2 = worst_ratio(Z[s, 2], ref["pd"][s], (c["dim"] + 8 + 2) * U * ref["pd"][s])
    return r1, r2


# ---- cdist_cosine ---------------------------------------------------------------------------------------------------------
CD_TABLE = ((1, 1, 1), (1, 13, 64), (1, 2, 257), (255, 1, 3), (255, 13, 256), (255, 33, 64), (255, 2, 1), (256, 1, 255),
            (256, 2, 64), (256, 13, 257), (256, 33, 3), (257, 1, 256), (257, 2, 255), (257, 13, 1), (257, 33, 257), (257, 13, 64))
CD_SAME = slice(100, 140)               # rows identical to row 99


def cd_cases():
    return [dict(i=i, n=n, k=k, dim=dim) for i, (n, k, dim) in enumerate(CD_TABLE)]


def cd_inputs(c):
    """rows around k centres; centroid 0 holds float32 values (a row can EQUAL it), centroid 1 is zero, the others are float64.
    n >= 255: row 5 NaN, row 6 zero, row 7 = centroid 0, row 8 = 3 centroid 0, rows 100..139 = row 99; n = 1: the row is 3
    centroid 0"""
    g = _seed("cd", c["i"])
    n, k, dim = c["n"], c["k"], c["dim"]
    cent = g.standard_normal((k, dim))
    cent[0] = cent[0].astype(F32)
    if k > 1:
        cent[1] = 0.0
    e = (cent[g.integers(0, k, n)] + 0.6 * g.standard_normal((n, dim))).astype(F32)
    c0 = cent[0].astype(F32)
    if n == 1:
        e[0] = c0 * F32(3)
    else:
        e[5], e[6], e[7], e[8] = np.nan, 0.0, c0, c0 * F32(3)
        e[CD_SAME] = e[99]
    return dict(e=e, cent=cent)


def cd_run(c, inp, ssum=seq_sum, mutant=None):
    """cdist_cosine_kernel's statement.  ssum = seq_sum: the kernel's order (THE reference of the device test)"""
    e, v = inp["e"].astype(F64), inp["cent"]
    vn = v.astype(F32).astype(F64) if mutant == "norm_f32" else v
    with np.errstate(all="ignore"):
        s = ssum(e[:, None, :] * v[None, :, :], 2)
        ne, nc = np.sqrt(ssum(e * e, 1)), np.sqrt(ssum(vn * vn, 1))
        pre = s / (ne[:, None] * nc[None, :])
        cos = pre if mutant == "no_clip" else np.where(np.abs(pre) > 1.0, np.copysign(1.0, pre), pre)
        out = 1.0 - cos
    if mutant == "row_mod_n":           # thread idx -> (idx % n, idx / n) where (idx / k, idx % k) is meant
        idx = np.arange(c["n"] * c["k"])
        out = out[idx % c["n"], idx // c["n"]].reshape(c["n"], c["k"])
    return dict(out=out, pre=pre, cos=cos)


def cd_exact(c, inp):
    """cos before the clip with longdouble sums, and sum|e v| / den"""
    e, v = inp["e"].astype(LD), inp["cent"].astype(LD)
    with np.errstate(all="ignore"):
        p = e[:, None, :] * v[None, :, :]
        den = np.sqrt((e * e).sum(1))[:, None] * np.sqrt((v * v).sum(1))[None, :]
        return dict(pre=(p.sum(2) / den), sabs=(np.abs(p).sum(2) / den).astype(F64))


def cd_bound(c, inp, s=1.0):
    return dict(out=8 * U * np.abs(cd_run(c, inp)["cos"]) + U)


def cd_check(c, inp, got, ref=None, bound=None):
    """worst error / bound of `got` [n, k]; inf when an EXACT property fails"""
    ref = cd_run(c, inp)["out"] if ref is None else ref
    bound = cd_bound(c, inp)["out"] if bound is None else bound
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return math.inf
    if c["n"] > 1 and not np.array_equal(got[CD_SAME].view(np.uint64), np.broadcast_to(got[99], got[CD_SAME].shape).copy().view(np.uint64)):
        return math.inf
    ok = ~nan
    if ((got[ok] < 0) | (got[ok] > 2)).any():
        return math.inf
    return worst_ratio(got[ok], ref[ok], bound[ok])


# ---- vbx ------------------------------------------------------------------------------------------------------------------
VB_E = (1, 3, 4, 5, 255, 256, 257, 513)
VB_K = (1, 7, 8, 9, 17)
VB_D = (1, 63, 64, 65, 128, 255, 256, 300)
VB_FA, VB_FB = 0.07, 0.8
VB_SAT_FACTOR = 3e3                     # the rows scaled so that one speaker leads by more than 745


def vb_cases():
    out = []
    for i in range(24):
        K = VB_K[i % 5]
        out.append(dict(i=i, E=VB_E[i // 3], K=K, D=VB_D[(3 * i) % 8], sat=K > 1 and i % 2 == 0, pi0=K > 1 and i % 3 == 1))
    return out


def vb_sums(name):
    """(sum over D of a dot product, sum over the E rows): exact (the reference), forward, or the kernels' own orders"""
    return {"exact": (exact_sum, exact_sum), "forward": (seq_sum, seq_sum), "kernel": (phase_sum(64), chunk_sum(256))}[name]


def _vb_stats(X, Phi, g, dt, srow, mutant=None):
    E, D = X.shape
    K = g.shape[1]
    rho = X.astype(dt) * np.sqrt(Phi.astype(dt))
    if mutant == "lane_tail":
        rho[:, 64 * (D // 64):] = 0
    gg = g.astype(dt)
    if mutant == "last_chunk_256" and E % 256:      # rows past E: whatever lies there; modelled as the first rows again
        extra = np.arange(E, 256 * -(-E // 256)) % E
        rho, gg = np.concatenate([rho, rho[extra]]), np.concatenate([gg, gg[extra]])
    st = np.zeros((K, D + 1), dt)
    for k in range(K):
        st[k, :D] = srow(gg[:, k:k + 1] * rho, 0)
    st[:, D] = srow(gg, 0)
    if mutant == "ns_col":
        st[:, D] = st[:, D - 1]
    if mutant == "tile0":
        st[8:] = st[np.arange(8, K) % 8] if K > 8 else st[8:]
    return st


def vb_inputs(c):
    """oracle.gen_golden.synth_vbx_case's recipe with the case's D and K (K = 1: one speaker); sat: row 0 (and row E // 2) scaled
    by VB_SAT_FACTOR.  The smoothed one-hot responsibilities get a 5 % jitter: hundreds of IDENTICAL terms added in forward order
    round the same way every time (a systematic error, inside (n + 8) u but not inside a quarter of it), which says nothing about
    the share an ideal kernel needs on data that is not made of copies.  alpha, ck and lpi are GIVEN: clustering.vb_gmm's expressions on the exact statistics, pi uniform or, with
    pi0, zero for the last speaker"""
    from scipy.special import softmax
    r = _seed("vb", c["i"])
    E, K, D = c["E"], c["K"], c["D"]
    nspk = max(K - 1, 1)
    mu = 3.0 * r.standard_normal((nspk, D))
    lab = r.integers(0, nspk, E)
    X = mu[lab] + r.standard_normal((E, D))
    if c["sat"]:
        X[[0, E // 2]] *= VB_SAT_FACTOR
    Phi = np.abs(r.standard_normal(D)) * 2.0 + 0.05
    q0 = np.zeros((E, K))
    q0[np.arange(E), np.where(r.random(E) < 0.15, r.integers(0, K, E), lab)] = 1.0
    g0 = softmax(q0 * 7.0 + 0.05 * r.standard_normal((E, K)), axis=1)     # jitter: see the docstring
    st =_vb_stats(X, Phi, g0, LD, exact_sum).astype(F64)
    invL = 1.0 / (1 + VB_FA / VB_FB * st[:, D:D + 1] * Phi)
    alpha = VB_FA / VB_FB * invL * st[:, :D]
    ck = 0.5 * (invL + alpha ** 2).dot(Phi)
    pi = np.ones(K) / K
    if c["pi0"]:
        pi = np.append(np.ones(K - 1) / (K - 1), 0.0)
    return dict(X=X, Phi=Phi, g0=g0, alpha=alpha, ck=ck, lpi=np.log(pi + 1e-8))


def vb_run(c, inp, dt=LD, sums="exact", mutant=None):
    """stats() right after create, then ONE estep() with the given alpha / ck / lpi: dict(stats, gamma, total, a, l)"""
    sdot, srow = vb_sums(sums)
    E, K, D = c["E"], c["K"], c["D"]
    X, Phi = inp["X"].astype(dt), inp["Phi"].astype(dt)
    st = _vb_stats(inp["X"], inp["Phi"], inp["g0"], dt, srow, mutant)
    Dd = 64 * (D // 64) if mutant == "lane_tail" else D
    rho = (X * np.sqrt(Phi))[:, :Dd]
    G = dt(-0.5) * (sdot(X[:, :Dd] * X[:, :Dd], 1).astype(dt) + dt(D) * dt(LOG_2PI)) if Dd else np.full(E, dt(-0.5) * dt(D) * dt(LOG_2PI))
    alpha, ck, lpi, Fa = inp["alpha"].astype(dt), inp["ck"].astype(dt), inp["lpi"].astype(dt), dt(VB_FA)
    dot = np.stack([sdot(rho * alpha[k, :Dd], 1).astype(dt) if Dd else np.zeros(E, dt) for k in range(K)], 1)
    a = Fa * (dot - ck + G[:, None]) + lpi
    with np.errstate(all="ignore"):
        if mutant == "no_shift":
            l = np.log(sdot(np.exp(a), 1).astype(dt))
        else:
            amax = a.max(1)
            l = np.log(sdot(np.exp(a - amax[:, None]), 1).astype(dt)) + amax
        gamma = np.exp(a - l[:, None])
        total = srow(l, 0)
    return dict(stats=st, gamma=gamma, total=total, a=a, l=l, dot=dot, G=G)


def vb_bound(c, inp, s=1.0):
    E, K, D = c["E"], c["K"], c["D"]
    X, Phi, g0 = inp["X"], inp["Phi"], inp["g0"]
    ref = vb_run(c, inp)
    rho = X * np.sqrt(Phi)
    sgr = np.concatenate([g0.T @ np.abs(rho), g0.sum(0)[:, None]], 1)               # sum|gamma rho| and sum gamma
    bst = (E + 8) * s * U * sgr
    bst[:, :D] += 3 * U * sgr[:, :D]
    sx2 = (X * X).sum(1)
    G = ref["G"].astype(F64)
    dG = 0.5 * ((D + 8) * s * U * sx2 + U * D * LOG_2PI) + 2 * U * np.abs(G)
    S = np.abs(rho) @ np.abs(inp["alpha"]).T                                          # [E, K]
    dot, a, l = ref["dot"].astype(F64), ref["a"].astype(F64), ref["l"].astype(F64)
    t1 = dot - inp["ck"]
    da = VB_FA * ((D + 8) * s * U * S + 3 * U * S + dG[:, None] + U * np.abs(t1) + U * np.abs(t1 + G[:, None])) \
        + U * np.abs(a - inp["lpi"]) + U * np.abs(a)
    lse = l - a.max(1)                                                                  # log of the sum of exponentials, >= 0
    dl = da.max(1) + ((K + 8) * s * U + 4 * U) + ULP_FN + ULP_FN * np.abs(lse) + U * np.abs(l)
    gam = ref["gamma"].astype(F64)
    with np.errstate(over="ignore"):
        bg = gam * np.expm1(da + dl[:, None] + U * np.abs(a - l[:, None]) + ULP_FN) + 2.0 ** -1072
    lead = np.sort(a, 1)
    sat = (lead[:, -1] - lead[:, -2] > 745.0) if K > 1 else np.zeros(E, bool)
    return dict(stats=bst, gamma=bg, total=(E + 8) * s * U * np.abs(l).sum() + dl.sum(), rowsum=(K + 8) * U + bg.sum(1), sat=sat)


def vb_check(c, ref, bnd, got):
    """worst error / bound over stats, gamma, the rows' sums and the total; inf where a saturated row is not exactly 0 / 1"""
    r = max(worst_ratio(got["stats"], ref["stats"].astype(F64), bnd["stats"]), worst_ratio(got["gamma"], ref["gamma"].astype(F64), bnd["gamma"]),
            worst_ratio(np.asarray(got["gamma"], F64).sum(1), np.ones(c["E"]), bnd["rowsum"]),
            worst_ratio(got["total"], F64(ref["total"]), bnd["total"]))
    g = np.asarray(got["gamma"], F64)[bnd["sat"]]
    if g.size and not (np.isin(g, (0.0, 1.0)).all() and (g.sum(1) == 1.0).all()):
        return math.inf
    return r


# ---- prepare_masks --------------------------------------------------------------------------------------------------------
PM_L = (1, 2, 3, 5, 6, 10, 11, 12, 255, 256, 257, 799)
PM_S = (1, 2, 3, 4, 8)
PM_MEDIAN = (1, 3, 11, 21)
PM_FRAME = {1: 1, 2: 2, 3: 2, 4: 2, 8: 1}          # max_speakers_per_frame of the engine built for S (<= 16 powerset classes)
PM_SCIPY_OUTSIDE = (2, 21)              # (L, median) at which scipy itself leaves the signal: see the docstring
PM_LDS_OK, PM_LDS_REFUSED = (4094, 8), (4095, 8)    # 2 round4(L S) + 32 <= 65536 and the first L past it


def pm_cases():
    out = []
    for i, L in enumerate(PM_L):
        for j in range(3):
            out.append(dict(L=L, S=PM_S[(i + 2 * j) % 5], median=PM_MEDIAN[(i + j) % 4]))
    for L, S in ((3, 4), (3, 3), (5, 8), (6, 2), (10, 1)):                  # windows longer than the signal, twice and more
        out.append(dict(L=L, S=S, median=21))
    for c in out:
        if (c["L"], c["median"]) == PM_SCIPY_OUTSIDE:
            c["median"] = 11
    out.append(dict(L=2, S=3, median=11))
    for i, c in enumerate(out):
        L = c["L"]
        c.update(i=i, B=(1, 3)[i % 2], exclude_overlap=(i // 2) % 2, min_num_frames=(0, 1, L)[i % 3], want_masks=i != 7)
    return out


def pm_inputs(c, B=None):
    g = _seed("pm", c["i"])
    B, L, S = B or c["B"], c["L"], c["S"]
    raw = (g.random((B, L, S)) > 0.55).astype(np.uint8)
    if S >= 2 and L >= 10:
        raw[0, :, 1] = raw[0, :, 0]                 # an almost always overlapped speaker
    if S >= 3:
        raw[-1, :, 2] = 0                           # a silent one
    return dict(raw=raw)


def pm_index(L, median, mutant=None):
    """[L, median]: the frame every tap of every output frame reads"""
    tt = np.arange(L)[:, None] + np.arange(-(median // 2), median // 2 + 1)[None, :]
    if mutant == "reflect_once":        # the rule before this matrix: one reflection, then a clamp
        tt = np.where(tt < 0, -tt - 1, tt)
        tt = np.where(tt >= L, 2 * L - tt - 1, tt)
        return np.clip(tt, 0, L - 1)
    m = np.mod(tt, 2 * L)
    return np.where(m < L, m, 2 * L - 1 - m)


def _pm_masks(c, fil):
    f = fil.astype(F32)
    clean = f * (f.sum(axis=2, keepdims=True) < 2)
    B, _, S = f.shape
    use = c["exclude_overlap"] and True
    m = np.stack([[clean[b, :, s] if use and clean[b, :, s].sum() > c["min_num_frames"] else f[b, :, s] for s in range(S)] for b in range(B)])
    return m.astype(F32)


def pm_run(c, inp, mutant=None):
    """the kernel's index rule in numpy: a majority vote over the taps"""
    raw = inp["raw"]
    fil = raw if c["median"] <= 1 else (raw[:, pm_index(c["L"], c["median"], mutant), :].sum(2) > c["median"] // 2).astype(np.uint8)
    return dict(filtered=fil, masks=_pm_masks(c, fil))


def pm_ref(c, inp):
    from scipy.ndimage import median_filter
    fil = median_filter(inp["raw"].astype(F32), size=(1, c["median"], 1), mode="reflect").astype(np.uint8)
    return dict(filtered=fil, masks=_pm_masks(c, fil))


# ---- speaker_count / cluster_activations ----------------------------------------------------------------------------------
AG_C, AG_L, AG_S, AG_K = (0, 1, 2, 7), (1, 5, 99), (1, 3, 8), (1, 2, 31, 32)
AG_STRIDE = dict(C=5300, L=399, S=2, K=2)           # C L = 2 114 700 > 8192 * 256: the grid-stride loop takes a second pass


def ag_cases():
    out = []
    for i in range(12):
        out.append(dict(i=i, kind="random", C=AG_C[i % 4], L=AG_L[i % 3], S=AG_S[(i // 2) % 3], K=AG_K[(i + i // 4) % 4]))
    out.append(dict(i=12, kind="halves", C=2, L=5, S=3, K=2))
    out.append(dict(i=13, kind="stride", **AG_STRIDE))
    return out


def ag_inputs(c):
    g = _seed("ag", c["i"])
    C, L, S, K = c["C"], c["L"], c["S"], c["K"]
    if c["kind"] == "halves":           # sum / cnt = 0.5, 1.5, 2.5 on frames 0, 1, 2 -> 0, 2, 2; frames 3, 4: 1 and 0; 5, 6 uncovered
        seg = np.zeros((2, 5, 3), np.uint8)
        seg[0, :4, 0] = 1
        seg[0, 1:3, 1] = 1
        seg[0, 2, 2] = 1
        seg[1, 1:4, 0] = 1
        seg[1, 2, 1] = 1
        return dict(seg=seg, start=np.zeros(2, np.int32), hard=np.array([[0, 0, 1], [1, -2, 1]], np.int8), T=7)
    if c["kind"] == "stride":
        start = (3 * np.arange(C)).astype(np.int32)
        T = int(start[-1]) + L - 50                 # the last windows run past T
    else:
        T = C * L + 2 * L + 5                       # room for frames no window covers
        start = np.sort(g.integers(-L, T, C)).astype(np.int32)
        if C >= 1:
            start[0] = -(L // 2) - 1                # cut by t < 0 (L = 1: wholly outside)
        if C >= 2:
            start[-1] = T - L // 2                  # cut by t >= T (L = 1: wholly outside)
    seg = (g.random((max(C, 1), L, S)) < 0.5).astype(np.uint8)
    hard = g.integers(-2, K + 1, (max(C, 1), S)).astype(np.int8)      # -2, -1 and K among the labels
    if S >= 2:
        hard[:, 1] = hard[:, 0] = g.integers(0, K, max(C, 1))         # two local speakers on one cluster
    if S >= 3 and C >= 2:
        hard[0, 2], hard[1, 2] = K, -1
    return dict(seg=seg, start=start, hard=hard, T=T)


def ag_run(c, inp, mutant=None):
    """dict(count u8 [T], act i32 [T, K]) in integer numpy; np.rint in float32 is half to even like rintf"""
    C, L, S, K, T = c["C"], c["L"], c["S"], c["K"], inp["T"]
    seg, hard = inp["seg"][:C].astype(np.int64), inp["hard"][:C].astype(np.int64)
    t = inp["start"][:C, None].astype(np.int64) + np.arange(L)[None, :]                # [C, L]
    if mutant == "past_T":              # t >= T not skipped: modelled as landing on the last frame
        keep, t = t >= 0, np.minimum(t, T - 1)
    else:
        keep = (t >= 0) & (t < T)
    ssum, cnt = np.zeros(T, np.int64), np.zeros(T, np.int64)
    np.add.at(ssum, t[keep], seg.sum(2)[keep])
    np.add.at(cnt, t[keep], 1)
    with np.errstate(all="ignore"):
        avg = np.where(cnt > 0, ssum.astype(F32) / np.maximum(cnt.astype(F32), F32(1e-12)), F32(0)).astype(F32)
    count = (np.floor(avg + F32(0.5)) if mutant == "floor_half" else np.rint(avg)).astype(np.uint8)
    kmax = K + 1 if mutant == "label_K" else K
    flat = np.zeros(T * K + K + 1, np.int64)        # a label equal to K lands on the next frame's cluster 0
    for k in range(kmax):
        sel = (hard == k)[:, None, :] & (seg > 0)                                        # [C, L, S]
        v = sel.sum(2) if mutant == "sum" else sel.any(2).astype(np.int64)
        np.add.at(flat, (t * K + k)[keep], v[keep])
    return dict(count=count, act=flat[:T * K].reshape(T, K).astype(np.int32))


# ---- hysteresis -----------------------------------------------------------------------------------------------------------
HY_N = (1, 2, 1023, 1024, 1025, 2049)
HY_THR = ((0.5, 0.5), (0.6, 0.4), (1.0, 0.0))
HY_THREADS = 1024


def hy_cases():
    out = []
    for n in HY_N:
        for onset, offset in HY_THR:
            out.append(dict(i=len(out), n=n, onset=onset, offset=offset, t0=0, entry=None))
            if n >= 2:
                for entry in (0, 1):
                    out.append(dict(i=len(out), n=n, onset=onset, offset=offset, t0=(1, n // 3 + 1)[entry], entry=entry))
    return out


def hy_inputs(c):
    """two windows at start 0 with L = n, one speaker each, weights 1: the score of frame t is (seg[0, t] + seg[1, t]) / 2.  Runs of
    1 .. 40 equal frames, three in five of them at 0.5: undecided stretches longer than several threads' chunks (<= 3 frames)"""
    g = _seed("hy", c["n"])
    n = c["n"]
    v = np.zeros(0, np.int64)
    while len(v) < n:
        v = np.concatenate([v, np.full(g.integers(1, 41), g.choice(3, p=(0.2, 0.6, 0.2)))])
    v = v[:n]
    seg = np.stack([v >= 1, v >= 2]).astype(np.uint8).reshape(2, n, 1)
    return dict(seg=seg, y=(v.astype(F32) * F32(0.5)))


def hy_run(c, inp, mutant=None):
    """postprocess._hysteresis over frames [t0, n); for t0 > 0 the entry state is a decisive frame put in front"""
    from diarizen_amd.postprocess import _hysteresis
    y, t0 = inp["y"], c["t0"]
    on, off = F32(c["onset"]), F32(c["offset"])
    if mutant == "non_strict":
        on, off = np.nextafter(on, F32(-1)), np.nextafter(off, F32(2))
    if t0 == 0:
        return dict(active=_hysteresis(y, on, off).astype(np.uint8), scores=y)
    lead = F32(2.0 if c["entry"] else -1.0)
    return dict(active=_hysteresis(np.concatenate([[lead], y[t0:]]).astype(F32), on, off)[1:].astype(np.uint8), scores=y[t0:])
