"""Shared by test_small_kernels_gpu.py (device) and test_small_kernels_host.py (CPU): case tables, inputs, float64 references
and per-element error bounds of the kernels between the contractions and the attention family — csrc/conformer.hip
(glu_dwconv, classify), csrc/frontend.hip (groupnorm_gelu, pad_rows, ws_accum, ws_sum, col_scale), csrc/norm.hip (layernorm_t,
wave_stats) and csrc/embed.hip (frame_prep, power, log_cmn, log_cmn_gather, stem_conv, stats_pool, window_active,
compact_active).  numpy (+ torch.erf); nothing here touches a device.

Every kernel has ONE function `<k>_run(case, inp, dt, ssum, mutant)` that states the operation as the reference project defines
it (the kernel comments name the lines).  With dt = float64 and the exact sum it is the reference; with dt = float32 and a
sequential sum (`seq_sum`: forward; `phase_sum(n)`: the kernel's n phases, then the phases in order) it is an IDEAL fp32 kernel,
every operation rounded once; with `mutant` it is one of the subtly wrong kernels test_small_kernels_host.py holds the bound
against.  `<k>_bound(case, inp)` is the per-element bound, DERIVED, never tuned.  u = 2^-24:

  sums            n terms t_i added in fp32 in ANY order: (n + 8) u sum|t_i|, as _gemm_cases.py counts an accumulation.  The
                  kernels' own chains are shorter (phases, cross-lane trees), but the next rewrite will reorder them and the bound
                  must not care: n counts TERMS.  This is the ACCUMULATION share of a bound; every bound function takes a factor
                  `s` on it, and test_small_kernels_host.py shows that an ideal fp32 kernel stays inside the bound at s = 1/4 (a
                  factor 4 inside the accumulation share; single roundings enter at face value, as in the other two matrices).
  expf, logf      2 ulp = 4 u relative ("a few ulp"; ULP_FN).  sqrtf and the divisions: 1 ulp = 2 u.
  sigmoid         1 / (1 + expf(-x)): 4 u + 2 u -> 6 u relative, and 2^-126 absolute where expf overflows (x < -88.7: the kernel
                  gives 0, the true value is a denormal).
  erf_as          1.5e-7 absolute by its formula (Abramowitz & Stegun 7.1.26) + 8 u: one u for each of the eight fp32 operations
                  that evaluate it, as _gemm_cases.py counts it.  gelu(x) = x (1 + erf(x / sqrt 2)) / 2: |x| / 2 times that (+ 4 u for
                  the constant and the product inside), 3 u relative for the three products outside; |gelu'| <= 1.13.
  normalisations  mean: K u mean|x|, K = (n + 8) s.  Two passes: the centred sum of squares M2
                  carries (K + 3) u M2 + n dmu^2 (a wrong centre adds n dmu^2 exactly); var = M2 / n; rstd = (var + eps)^-1/2
                  moves by rstd (dvar / (2 (var + eps)) + 3 u): its sensitivity to the variance error + division, sqrt, division.

glu_dwconv   g = a sigmoid(b): e_g = 8 u |g| + 2^-125 |a|.  acc = sum_j g_j w_j + bias: (ks + 1 + 8) s u (sum|g_j w_j| + |bias|) + sum|w_j|
             e_g,j.  out = acc sigmoid(acc): 1.1 d_acc (|swish'| <= 1.1) + 8 u |out| + 2^-125 |acc|.
classify     logit: (A + 1 + 8) s u (sum|z w| + |bias|).  log-sum-exp is
             1-Lipschitz in the logits' sup norm: d_lse = max_c d_l + (u max|l - mx| + 4 u + (NC + 8) s u) (relative error of the sum
             of exponentials, which is >= 1) + 4 u |log se| + u |lse|.  logp: d_l + d_lse + u |logp|.  soft_s = sum_{c has s}
             exp(l_c - lse): every term off by the factor exp(r_c), r_c = d_l,c + d_lse + u |l_c - lse| + 4 u, + (NC + 8) s u for the adds.
             multilabel: exact, except rows whose float64 top-two gap (between classes that are not bit-identical copies of each
             other) is below 2 max_c d_l; at most 1 % of the rows of a case (checked on the CPU).
groupnorm    K = (T + 8 + 4 nchunk) s (the T rows; Chan's merge: four roundings per 128-row chunk).  pre = (x - mu) rstd gamma + beta:
             |rstd gamma| (dmu + u |x - mu|) + |pre - beta| (drstd + 2 u) + u |pre|, then the GELU terms.
layernorm    K = (C + 8) s.  Then as above;
             post: one more product.  The tracker is compared EXACTLY with the maximum of the |y| the kernel stored.
wave_stats   K = (N + 8) s.
frame_prep   v = 2^15 x exact; mean: K = (flen + 8) s.  r = (v - m) - p (v' - m) = v - p v' - (1 - p) m: (1 - p) dmu + 2 u |v - m| +
             3 u p |v' - m| + u |r|; times the window: |w| d_r + u |out|.
power        (re^2 + im^2 -> sqrt -> square): 2 u, then u + 2 u, doubled + u = 7 u -> 8 u |pw| + 2^-124.
log_cmn      v = logf(max(m, eps)): 4 u |v|; mean over T: K = (T + 8) s -> (K u + 4 u) mean|v|; out = v - mean: u |out|.
             log_cmn_gather: the same BITS as log_cmn on a copy of the window's rows.
stem_conv    nine fmas: (9 + 8) s u sum|in w|; the bias: u (sum|in w| + |bias|); ReLU is 1-Lipschitz.
ws_accum / ws_sum  product, then add (no contraction): an fp32 emulation gives the same BITS; against float64 ((k + 8) s + 1) u sum|w x| (the adds; the products).
pad_rows, col_scale, window_active, compact_active: exact (col_scale: one correctly rounded product = numpy's).
stats_pool   w = mask[src(t)], src = min(floor(fl(t) fl(L / W)), L - 1) in fp32 (torch's nearest), v1 = sum w + 1e-8,
             mean = sum(x w) / v1: (k sum|x| w + |mean| k v1) / v1, k = (W + 8) s u, + u |mean|.  N = sum d^2 w with d = x - mean:
             sum w (2 |d| e_d + e_d^2 + 3 u d^2) + k N, e_d = dmean + u |d|.  D = v1 - v2 / v1 + 1e-8 CANCELS: dD = dv1 +
             (v2 / v1) (k + 2 u + dv1 / v1) + u |v1 - v2 / v1| + u D.  var in [max(N - dN, 0) / (D + dD), (N + dN) / (D - dD)],
             std = sqrt(var): the interval's ends (+ 2 u each for division and sqrt).  Where D - dD <= 0 fp32 cannot resolve the
             denominator (ONE non-zero frame of weight 1: D = 1e-8 in fp32, 3e-8 in float64): the bound is infinite and the
             test only asks for a finite, non-negative number there; the mean is bounded everywhere.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
ULP_FN = 4 * U
ERF_ABS = 1.5e-7 + 8 * U
PATTERN = 0x7FA5C3C3            # NaN as fp32: an element nobody stored is not finite
GUARD = 1024                    # elements of band before and after every buffer
F32, F64 = np.float32, np.float64
EPS_LN = float(np.float32(1e-5))        # the launchers take eps as a float


# ---- sums -----------------------------------------------------------------------------------------------------------------
def exact_sum(x, axis):
    return np.sum(x, axis=axis)


def seq_sum(x, axis):
    return np.take(np.add.accumulate(x, axis=axis, dtype=x.dtype), -1, axis=axis)


def rev_sum(x, axis):
    return seq_sum(np.flip(x, axis), axis)


def phase_sum(nph):
    """element t belongs to phase t % nph; a phase adds its elements in order, then the phases are added in order"""
    def f(x, axis):
        x = np.moveaxis(x, axis, 0)
        pad = (-x.shape[0]) % nph
        if pad:
            x = np.concatenate([x, np.zeros((pad,) + x.shape[1:], x.dtype)])
        return seq_sum(seq_sum(x.reshape((-1, nph) + x.shape[1:]), 0), 0)
    return f


def erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def gelu(x):
    t = x.dtype.type
    return (t(0.5) * x * (t(1) + erf(x * t(0.7071067811865476)))).astype(x.dtype)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return (x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))).astype(x.dtype)


def _seed(name, i):
    return np.random.default_rng([sum(map(ord, name)), i])


# ---- glu_dwconv -----------------------------------------------------------------------------------------------------------
def dw_cases():
    out = []
    for i, (ks, L, A) in enumerate(itertools.product((7, 15, 31), (1, 5, 31, 32, 33, 65), (20, 64, 100, 128, 192, 256, 320))):
        s = i % 2
        out.append(dict(i=i, B=3, L=L, A=A, ks=ks, ldu=2 * A + 8 * s, ldo=A + 4 * s))
    return out


def dw_inputs(c):
    g = _seed("dw", c["i"])
    B, L, A, ks = c["B"], c["L"], c["A"], c["ks"]
    a = g.standard_normal((B, L, A))
    a[1] *= 1024.0                                          # window 1 loud, its neighbours quiet
    b = 3.0 * g.standard_normal((B, L, A))
    sat = g.random((B, L, A))
    b[sat < 0.03] = 90.0
    b[sat > 0.97] = -90.0
    return dict(u=np.concatenate([a, b], 2).astype(F32), w=(g.standard_normal((A, ks)) / math.sqrt(ks)).astype(F32),
                bias=(0.1 * g.standard_normal(A)).astype(F32))


def _dw_taps(gv, B, L, A, ks, mutant):
    pad = (ks - 1) // 2
    if mutant == "halo_neighbour":                          # the halo of a window read from the rows next to it
        flat = np.concatenate([np.zeros((pad, A), gv.dtype), gv.reshape(B * L, A), np.zeros((pad + 1, A), gv.dtype)])
        gp = np.stack([flat[b * L:b * L + L + 2 * pad + 1] for b in range(B)])
    else:
        gp = np.concatenate([np.zeros((B, pad, A), gv.dtype), gv, np.zeros((B, pad + 1, A), gv.dtype)], 1)
    sh = 1 if mutant == "tap_shift" else 0
    return [gp[:, j + sh:j + sh + L, :] for j in range(ks)]


def dw_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    B, L, A, ks = c["B"], c["L"], c["A"], c["ks"]
    u = inp["u"].astype(dt)
    gv = u[..., :A] * sigmoid(u[..., A:])
    w = inp["w"].astype(dt)
    acc = ssum(np.stack([t * w[:, j] for j, t in enumerate(_dw_taps(gv, B, L, A, ks, mutant))]), 0) + inp["bias"].astype(dt)
    return dict(out=(acc * sigmoid(acc)).astype(dt))


def dw_bound(c, inp, s=1.0):
    B, L, A, ks = c["B"], c["L"], c["A"], c["ks"]
    u = inp["u"].astype(F64)
    a = u[..., :A]
    gv = a * sigmoid(u[..., A:])
    eg = 8 * U * np.abs(gv) + 2 * TINY * np.abs(a)
    w = np.abs(inp["w"].astype(F64))
    s_abs = sum(np.abs(t) * w[:, j] for j, t in enumerate(_dw_taps(gv, B, L, A, ks, None)))
    s_eg = sum(t * w[:, j] for j, t in enumerate(_dw_taps(eg, B, L, A, ks, None)))
    r = dw_run(c, inp)["out"]
    acc = sum(t * inp["w"].astype(F64)[:, j] for j, t in enumerate(_dw_taps(gv, B, L, A, ks, None))) + inp["bias"].astype(F64)
    d_acc = (ks + 1 + 8) * s * U * (s_abs + np.abs(inp["bias"].astype(F64))) + s_eg
    return dict(out=1.1 * d_acc + 8 * U * np.abs(r) + 2 * TINY * np.abs(acc))


# ---- classify -------------------------------------------------------------------------------------------------------------
POWERSETS = {(1, 1): 0, (4, 2): 2, (7, 3): 2, (11, 4): 2, (16, 4): 4}      # (NC, S) -> largest set size


def powerset_mapping(S, max_set):
    """row per class = the speakers of the set; classes ordered by set size, then lexicographically (Powerset.build_mapping)"""
    rows = []
    for k in range(max_set + 1):
        for comb in itertools.combinations(range(S), k):
            r = np.zeros(S, np.uint8)
            r[list(comb)] = 1
            rows.append(r)
    return np.stack(rows)


def cls_cases():
    out = []
    for i, (A, (NC, S), rows) in enumerate(itertools.product((20, 64, 100, 256), POWERSETS, (1, 3, 4, 5, 1027))):
        out.append(dict(i=i, A=A, NC=NC, S=S, rows=rows, ldz=A + 3 * (i % 2), null=(None, "logp", "multilabel", "soft")[i % 4]))
    return out


def cls_inputs(c):
    g = _seed("cls", c["i"])
    A, NC, S = c["A"], c["NC"], c["S"]
    W = 3.0 * g.standard_normal((NC, A)) / math.sqrt(A)
    b = g.standard_normal(NC)
    if NC >= 2:                                             # bit-identical classes: exact ties whenever one of them wins
        W[NC - 1], b[NC - 1] = W[0], b[0]
    if NC >= 4:
        W[2], b[2] = W[1], b[1]
    m = powerset_mapping(S, POWERSETS[(NC, S)])
    assert m.shape == (NC, S)
    return dict(z=g.standard_normal((c["rows"], A)).astype(F32), W=W.astype(F32), bias=b.astype(F32), mapping=m)


def cls_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    z, W, b, m = inp["z"].astype(dt), inp["W"].astype(dt), inp["bias"].astype(dt), inp["mapping"]
    NC = c["NC"]
    logit = np.stack([ssum(z * W[k], 1) for k in range(NC)], 1) + b
    arg = np.argmax(logit, 1)                               # the first maximum
    if mutant == "last_tie":
        arg = NC - 1 - np.argmax(logit[:, ::-1], 1)
    mx = logit.max(1, keepdims=True)
    lse = mx + np.log(ssum(np.exp(logit - mx), 1))[:, None]
    mm = m.astype(dt)
    if mutant == "soft_extra":                              # a class that does not hold speaker 0 enters its sum
        mm = mm.copy()
        mm[0, 0] = 1
    p = np.exp(logit - lse)
    soft = np.stack([ssum(p * mm[:, s], 1) for s in range(c["S"])], 1)
    return dict(logit=logit, logp=(logit - lse).astype(dt), multilabel=m[arg], soft=soft.astype(dt), arg=arg)


def cls_bound(c, inp, s=1.0):
    z, W, b = inp["z"].astype(F64), inp["W"].astype(F64), inp["bias"].astype(F64)
    NC, A = c["NC"], c["A"]
    r = cls_run(c, inp)
    l = r["logit"]
    dl = (A + 1 + 8) * s * U * (np.abs(z) @ np.abs(W).T + np.abs(b))
    dmax = dl.max(1, keepdims=True)
    mx = l.max(1, keepdims=True)
    se = np.exp(l - mx).sum(1, keepdims=True)
    lse = mx + np.log(se)
    dlse = dmax + (U * np.abs(l - mx).max(1, keepdims=True) + ULP_FN + (NC + 8) * s * U) + ULP_FN * np.abs(np.log(se)) + U * np.abs(lse)
    dlogp = dl + dlse + U * np.abs(r["logp"])
    rc = dl + dlse + U * np.abs(l - lse) + ULP_FN
    p = np.exp(l - lse)
    dsoft = (p * np.expm1(rc)) @ inp["mapping"].astype(F64) + (NC + 8) * s * U * r["soft"]
    # rows whose decision fp32 may not resolve: the gap to the best class that is not a bit-identical copy of the winner
    same = np.array([[np.array_equal(inp["W"][i], inp["W"][j]) and inp["bias"][i] == inp["bias"][j] for j in range(NC)] for i in range(NC)])
    other = np.where(same[r["arg"]], -np.inf, l)
    gap = l[np.arange(len(l)), r["arg"]] - other.max(1)
    return dict(logp=dlogp, soft=dsoft, unresolved=gap < 2 * dmax[:, 0])


# ---- groupnorm_gelu -------------------------------------------------------------------------------------------------------
GN_ROWS = 128


def gn_cases():
    out = []
    for j, (C, Cp) in enumerate(((4, 4), (30, 32), (153, 160), (512, 512), (1024, 1024))):
        for i, T in enumerate((1, 2, 127, 128, 129, 257, 385)):
            out.append(dict(i=7 * j + i, B=2, T=T, C=C, Cp=Cp, ld=Cp + 8 * ((i + j) % 2), inplace=bool(i & 1), amax=bool((i >> 1) & 1)))
    return out


def gn_inputs(c):
    g = _seed("gn", c["i"])
    B, T, C, Cp = c["B"], c["T"], c["C"], c["Cp"]
    x = g.standard_normal((B, T, C)) * (0.5 + g.random(C)) + 0.3 * g.standard_normal(C)
    x[:, :, 0] = 1e3 + g.standard_normal((B, T))            # the channel the two-pass form exists for
    x[:, :, 1] = 0.75                                       # a constant channel
    xp = np.full((B, T, Cp), 7.0)
    xp[..., :C] = x
    return dict(x=xp.astype(F32), gamma=(1 + 0.3 * g.standard_normal(C)).astype(F32), beta=(0.3 * g.standard_normal(C)).astype(F32))


def gn_stats(x, dt, ssum, chunked, mutant=None):
    """(mean, M2) over axis 1 of x [B, T, C]; chunked: GN_ROWS-row chunks, two passes inside, Chan's merge across"""
    T = x.shape[1]
    if not chunked:
        mean = ssum(x, 1) / dt(T)
        return mean, ssum((x - mean[:, None]) ** 2, 1)
    mean = np.zeros((x.shape[0], x.shape[2]), dt)
    m2, cnt = mean.copy(), dt(0)
    for r0 in range(0, T, GN_ROWS):
        xk = x[:, r0:r0 + GN_ROWS]
        n = xk.shape[1]
        mu = ssum(xk, 1) * (dt(1) / dt(n))
        mk = ssum((xk - mu[:, None]) ** 2, 1)
        n = dt(GN_ROWS if mutant == "last_chunk_128" else n)
        delta, tot = mu - mean, cnt + n
        mean = mean + delta * (n / tot)
        m2 = m2 + mk + (dt(0) if mutant == "no_cross" else delta * delta * (cnt * n / tot))
        cnt = tot
    return mean, m2


def gn_run(c, inp, dt=F64, ssum=exact_sum, mutant=None, chunked=False):
    C, T = c["C"], c["T"]
    x = inp["x"].astype(dt)[..., :C]
    mean, m2 = gn_stats(x, dt, ssum, chunked or mutant is not None, mutant)
    rstd = dt(1) / np.sqrt(m2 / dt(T) + dt(EPS_LN))
    pre = (x - mean[:, None]) * rstd[:, None] * inp["gamma"].astype(dt) + inp["beta"].astype(dt)
    y = np.zeros(inp["x"].shape, dt)
    y[..., :C] = gelu(pre.astype(dt))
    return dict(y=y)


def gn_nph(c):
    return 256 // (c["Cp"] // 4)


def gn_bound(c, inp, s=1.0):
    C, T = c["C"], c["T"]
    x = inp["x"].astype(F64)[..., :C]
    nchunk = (T + GN_ROWS - 1) // GN_ROWS
    K = (T + 8 + 4 * nchunk) * s
    mu = x.mean(1, keepdims=True)
    dmu = K * U * np.abs(x).mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    rs = 1 / np.sqrt(var + EPS_LN)
    drs = 0.5 * ((K + 3) * U * var + dmu ** 2) / (var + EPS_LN) + 3 * U
    gam, bet = inp["gamma"].astype(F64), inp["beta"].astype(F64)
    n = (x - mu) * rs * gam
    pre = n + bet
    dpre = np.abs(rs * gam) * (dmu + U * np.abs(x - mu)) + np.abs(n) * (drs + 2 * U) + U * np.abs(pre)
    b = np.zeros(inp["x"].shape)
    b[..., :C] = 1.13 * dpre + 0.5 * np.abs(pre) * (ERF_ABS + 4 * U) + 3 * U * np.abs(gelu(pre))
    return dict(y=b)


# ---- layernorm_t ----------------------------------------------------------------------------------------------------------
LN_TABLE = {(16, 1), (16, 2), (16, 3), (16, 4), (32, 3), (32, 4), (64, 3), (64, 4)}
#            float4 form: which (G, NV) instantiation the pair reaches
LN_V4 = {(4, 4): (16, 1), (60, 64): (16, 1), (64, 64): (16, 1), (128, 128): (16, 2), (153, 160): (16, 3), (211, 224): (16, 4),
         (256, 256): (16, 4), (260, 260): (32, 3), (512, 512): (32, 4), (768, 768): (64, 3), (1024, 1024): (64, 4)}
LN_OFFSET = ((256, 256), (1024, 1024))                      # a 4-byte-offset view: the scalar form
LN_WIDE = ((1025, 1028), (2048, 2048))                      # C > 1024: the scalar form
LN_BIG = (17000, 64, 64)                                    # about 4 MB
LN_ITERS = (65600, 4, 4)                                    # 16400 wavefront steps of four rows: iters = 2 in layernorm_v4_kernel


def ln_dispatch(C, Cpad, aligned=True):
    """launch_layernorm_t's choice: (G, NV) of the float4 form, or None = the scalar form"""
    need = max(C, Cpad)
    if need & 3 or need > 1024 or not aligned:
        return None
    best, pick = 1 << 30, None
    for G in (16, 32, 64):
        nv = (need + 4 * G - 1) // (4 * G)
        if nv <= 4 and nv * 4 * G < best:
            best, pick = nv * 4 * G, (G, nv)
    return pick if pick in LN_TABLE else None


def ln_iters(rows, C, Cpad):
    G, _ = ln_dispatch(C, Cpad)
    steps = -(-rows // (64 // G))
    return min(max(steps // (2048 * 4), 1), 8)


def ln_cases():
    out, i = [], 0
    shapes = [(p, "v4") for p in LN_V4] + [(p, "offset") for p in LN_OFFSET] + [(p, "wide") for p in LN_WIDE]
    for (C, Cpad), path in shapes:
        for rows in (1, 3, 5, 77):
            out.append(dict(i=i, rows=rows, C=C, Cpad=Cpad, path=path, affine=("gb", "none", "g", "b")[i % 4], post=bool((i >> 1) & 1),
                            gelu=bool((i >> 2) & 1), inplace=bool((i // 3) & 1), amax_unit=(None, 0, 1, 7)[(i // 2) % 4],
                            pad=8 * (i % 2)))
            i += 1
    for rows, C, Cpad in (LN_BIG, LN_ITERS):
        out.append(dict(i=i, rows=rows, C=C, Cpad=Cpad, path="v4", affine="gb", post=True, gelu=True, inplace=False, amax_unit=7, pad=0))
        i += 1
    return out


def ln_inputs(c):
    g = _seed("ln", c["i"])
    rows, C = c["rows"], c["C"]
    x = 2.0 * g.standard_normal((rows, C)) + 0.5
    if rows >= 3:
        x[1] = 0.3                                          # a constant row
    return dict(x=x.astype(F32), gamma=(1 + 0.3 * g.standard_normal(C)).astype(F32) if "g" in c["affine"] else None,
                beta=(0.3 * g.standard_normal(C)).astype(F32) if "b" in c["affine"] else None,
                post=(0.5 + g.random(C)).astype(F32) if c["post"] else None)


def ln_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    C = c["C"]
    x = inp["x"].astype(dt)
    div = dt(c["Cpad"] if mutant == "div_cpad" else C)
    mean = (ssum(x, 1) / div)[:, None]
    var = (ssum((x - mean) ** 2, 1) / div)[:, None]
    o = (x - mean) * (dt(1) / np.sqrt(var + dt(EPS_LN)))
    if inp["gamma"] is not None:
        o = o * inp["gamma"].astype(dt)
    if inp["beta"] is not None:
        o = o + inp["beta"].astype(dt)
    if c["gelu"]:
        o = gelu(o.astype(dt))
    if inp["post"] is not None:
        o = o * inp["post"].astype(dt)
    return dict(y=o.astype(dt))


def ln_bound(c, inp, s=1.0):
    x = inp["x"].astype(F64)
    K = (c["C"] + 8) * s
    mu = x.mean(1, keepdims=True)
    dmu = K * U * np.abs(x).mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    rs = 1 / np.sqrt(var + EPS_LN)
    drs = 0.5 * ((K + 3) * U * var + dmu ** 2) / (var + EPS_LN) + 3 * U
    t = (x - mu) * rs
    d = rs * (dmu + U * np.abs(x - mu)) + np.abs(t) * (drs + U)
    if inp["gamma"] is not None:
        gam = inp["gamma"].astype(F64)
        d, t = np.abs(gam) * d + U * np.abs(t * gam), t * gam
    if inp["beta"] is not None:
        t = t + inp["beta"].astype(F64)
        d = d + U * np.abs(t)
    if c["gelu"]:
        d, t = 1.13 * d + 0.5 * np.abs(t) * (ERF_ABS + 4 * U) + 3 * U * np.abs(gelu(t)), gelu(t)
    if inp["post"] is not None:
        p = inp["post"].astype(F64)
        d, t = np.abs(p) * d + U * np.abs(t * p), t * p
    return dict(y=d)


# ---- wave_stats -----------------------------------------------------------------------------------------------------------
WS_N = (1, 63, 1023, 1024, 1025, 16000)


def wv_inputs(N):
    g = _seed("wv", N)
    return dict(w=(0.5 + 1e-3 * g.standard_normal((3, N))).astype(F32))       # a DC offset on a small signal


def wv_run(N, inp, dt=F64, ssum=exact_sum, mutant=None):
    w = inp["w"].astype(dt)
    mean = ssum(w, 1) / dt(N)
    var = ssum((w - mean[:, None]) ** 2, 1) / dt(N)
    return dict(stats=np.stack([mean, dt(1) / np.sqrt(var + dt(EPS_LN))], 1).astype(dt))


def wv_bound(N, inp, s=1.0):
    w = inp["w"].astype(F64)
    K = (N + 8) * s
    dmu = K * U * np.abs(w).mean(1)
    var = w.var(1)
    rs = 1 / np.sqrt(var + EPS_LN)
    return dict(stats=np.stack([dmu, rs * (0.5 * ((K + 3) * U * var + dmu ** 2) / (var + EPS_LN) + 3 * U)], 1))


# ---- ws_accum / ws_sum ----------------------------------------------------------------------------------------------------
WSUM_COUNTS = (1, 3, 4, 5, 25, 40)
WSUM_SIZES = (4, 1020, 1048580)


def wsum_weights(k):
    return (0.2 + _seed("wsw", k).random(k)).astype(F32)


def wsum_run(xs, ws, dt=F64):
    """((0 + w0 x0) + w1 x1) + ...: with dt = float32 the kernel's own roundings (product, then add)"""
    acc = np.zeros(xs[0].shape, dt)
    for x, w in zip(xs, ws):
        acc = acc + dt(w) * x.astype(dt)
    return acc


def wsum_bound(xs, ws, s=1.0):
    return ((len(xs) + 8) * s + 1) * U * sum(abs(float(w)) * np.abs(x.astype(F64)) for x, w in zip(xs, ws))


# ---- frame_prep -----------------------------------------------------------------------------------------------------------
PREEMPH = float(F32(0.97))


def fp_cases():
    out, i = [], 0
    for flen in (400, 64, 65, 512):
        for Kp in sorted({flen, 416, 512}):
            if Kp < flen:
                continue
            for T in (1, 3, 4, 5):
                fshift = 160 if flen == 400 else 24
                span = (T - 1) * fshift + flen
                out.append(dict(i=i, B=2, T=T, flen=flen, fshift=fshift, Kp=Kp, span=span, stride=span + (-37, 0, 51)[i % 3]))
                i += 1
    return out


def fp_inputs(c):
    g = _seed("fp", c["i"])
    n = c["stride"] * (c["B"] - 1) + c["span"]
    steps = np.repeat(g.uniform(-0.4, 0.4, n // 64 + 1), 64)[:n]            # a step at every multiple of 64
    k = np.arange(c["flen"])
    win = 0.54 - 0.46 * np.cos(2 * np.pi * k / max(c["flen"] - 1, 1))
    return dict(wave=(steps + 0.05 * g.standard_normal(n)).astype(F32), window=win.astype(F32))


def fp_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    B, T, flen, Kp = c["B"], c["T"], c["flen"], c["Kp"]
    idx = (np.arange(B)[:, None, None] * c["stride"] + np.arange(T)[None, :, None] * c["fshift"] + np.arange(flen))
    v = inp["wave"].astype(dt)[idx] * dt(32768)
    mean = (ssum(v, 2) / dt(flen))[..., None]
    prev = np.concatenate([v[..., :1], v[..., :-1]], 2)
    if mutant == "first_zero":
        prev[..., 0] = 0
    if mutant == "early64":                                 # the previous sample at a register boundary taken 64 samples early
        for k in range(64, flen, 64):
            prev[..., k] = v[..., max(k - 65, 0)]
    r = (v - mean) - dt(PREEMPH) * (prev - mean)
    out = np.zeros((B * T, Kp), dt)
    out[:, :flen] = (r * inp["window"].astype(dt)).reshape(B * T, flen)
    return dict(frames=out)


def fp_bound(c, inp, s=1.0):
    B, T, flen, Kp = c["B"], c["T"], c["flen"], c["Kp"]
    idx = (np.arange(B)[:, None, None] * c["stride"] + np.arange(T)[None, :, None] * c["fshift"] + np.arange(flen))
    v = inp["wave"].astype(F64)[idx] * 32768
    mean = v.mean(2, keepdims=True)
    dmu = (flen + 8) * s * U * np.abs(v).mean(2, keepdims=True)
    prev = np.concatenate([v[..., :1], v[..., :-1]], 2)
    r = (v - mean) - PREEMPH * (prev - mean)
    dr = (1 - PREEMPH) * dmu + 2 * U * np.abs(v - mean) + 3 * U * PREEMPH * np.abs(prev - mean) + U * np.abs(r)
    w = np.abs(inp["window"].astype(F64))
    b = np.zeros((B * T, Kp))
    b[:, :flen] = (w * dr + U * np.abs(r * w)).reshape(B * T, flen)
    return dict(frames=b)


# ---- power, log_cmn, log_cmn_gather ---------------------------------------------------------------------------------------
MEL_T = (1, 7, 16, 17, 100)
MEL_NB = (1, 15, 16, 17, 80)
MEL_EPS = float(np.finfo(F32).eps)


def mel_cases():
    return [dict(i=i, B=2, T=T, NB=NB) for i, (T, NB) in enumerate(itertools.product(MEL_T, MEL_NB))]


def pw_inputs(c):
    g = _seed("pw", c["i"])
    return dict(spec=(g.standard_normal((c["T"], 2 * c["NB"])) * np.exp(3 * g.standard_normal((c["T"], 1)))).astype(F32))


def pw_run(c, inp, dt=F64, ssum=None, mutant=None):
    s = inp["spec"].astype(dt)
    a = np.sqrt(s[:, :c["NB"]] ** 2 + s[:, c["NB"]:] ** 2)
    return dict(pw=(a * a).astype(dt))


def pw_bound(c, inp, s=1.0):
    return dict(pw=8 * U * pw_run(c, inp)["pw"] + 4 * TINY)


def cmn_inputs(c, rows=None):
    g = _seed("cmn", c["i"])
    shape = (c["B"], c["T"], c["NB"]) if rows is None else (rows, c["NB"])
    m = np.exp(3 * g.standard_normal(shape))
    sel = g.random(shape)
    m[sel < 0.05] = 1e-12                                    # below eps
    m[sel > 0.96] = 0.0
    return dict(mel=m.astype(F32))


def cmn_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    T = c["T"]
    v = np.log(np.maximum(inp["mel"].astype(dt), dt(MEL_EPS)))
    n = 16 * -(-T // 16) if mutant == "mean16" else T
    return dict(mel=(v - (ssum(v, 1) / dt(n))[:, None]).astype(dt))


def cmn_bound(c, inp, s=1.0):
    T = c["T"]
    v = np.log(np.maximum(inp["mel"].astype(F64), MEL_EPS))
    K = (T + 8) * s
    out = v - v.mean(1, keepdims=True)
    return dict(mel=ULP_FN * np.abs(v) + (K * U + ULP_FN) * np.abs(v).mean(1, keepdims=True) + U * np.abs(out))


# ---- stem_conv ------------------------------------------------------------------------------------------------------------
STEM = ((1, 1), (3, 2), (5, 37), (80, 9))                   # (NB, T)
STEM_C = 32
STEM_Z = (None, ([2, 0], 2), ([1, 2], 0))                   # (z_list, z_count)


def stem_inputs(NB, T):
    g = _seed("stem", 100 * NB + T)
    return dict(fb=(3 * g.standard_normal((3, T, NB))).astype(F32), w=(g.standard_normal((STEM_C, 9)) / 3).astype(F32),
                bias=(0.2 * g.standard_normal(STEM_C)).astype(F32))


def _stem_taps(fb, NB, T):
    """the nine shifted copies in[b, h, t] = fb[b, t + dw - 1, h + dh - 1], zero outside, as [9][B, NB, T]"""
    p = np.pad(fb, ((0, 0), (1, 1), (1, 1)))
    return [np.transpose(p[:, dw:dw + T, dh:dh + NB], (0, 2, 1)) for dh in range(3) for dw in range(3)]


def stem_run(NB, T, inp, dt=F64, ssum=exact_sum, mutant=None):
    w = inp["w"].astype(dt)
    taps = _stem_taps(inp["fb"].astype(dt), NB, T)
    acc = ssum(np.stack([t[..., None] * w[:, k] for k, t in enumerate(taps)]), 0) + inp["bias"].astype(dt)
    return dict(img=np.maximum(acc, dt(0)).astype(dt))      # interior [B, NB, T, C]


def stem_bound(NB, T, inp, s=1.0):
    w = np.abs(inp["w"].astype(F64))
    taps = _stem_taps(np.abs(inp["fb"].astype(F64)), NB, T)
    S = sum(t[..., None] * w[:, k] for k, t in enumerate(taps))
    return dict(img=(9 + 8) * s * U * S + U * (S + np.abs(inp["bias"].astype(F64))))


# ---- stats_pool -----------------------------------------------------------------------------------------------------------
POOL_SHAPES = ((1, 1, 32), (3, 13, 64), (10, 100, 256))     # (H, W, C)
POOL_MASKS = ("zero", "single", "soft", "inactive")


def pool_cases():
    out, i = [], 0
    for (H, W, C), S in itertools.product(POOL_SHAPES, (1, 4)):
        for L in dict.fromkeys((W, 2 * W - 1, 399, 799, 5)):
            out.append(dict(i=i, B=2, H=H, W=W, C=C, S=S, L=L, mask=POOL_MASKS[i % 4]))
            i += 1
    return out


def pool_src(W, L, mutant=None):
    """F.interpolate(mode="nearest") from L to W frames: the source index of frame t, in float32 as torch computes it"""
    if W == L:
        return np.arange(W)
    scale = F32(L) / F32(W)
    f = np.arange(W, dtype=F32) * scale
    src = np.rint(f) if mutant == "round" else np.floor(f)
    return np.minimum(src.astype(np.int64), L - 1)


def pool_inputs(c):
    g = _seed("pool", c["i"])
    B, H, W, C, S, L = c["B"], c["H"], c["W"], c["C"], c["S"], c["L"]
    img = np.abs(g.standard_normal((B, H, W, C))) + 0.1 * g.standard_normal((B, H, W, C))
    kind = c["mask"]
    if kind == "zero":
        m = np.zeros((B, S, L))
    elif kind == "single":
        m = np.zeros((B, S, L))
        for b, s in itertools.product(range(B), range(S)):
            m[b, s, g.integers(L)] = 1.0
    else:
        m = g.random((B, S, L)) * (g.random((B, S, L)) < 0.7)
    active = None
    if kind == "inactive":
        active = np.array([1, 0], np.int32)
        m[1] = 0
        img[1] = np.nan                                      # stale: never read
    return dict(img=img.astype(F32), masks=m.astype(F32), active=active)


def pool_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    B, H, W, C, S, L = c["B"], c["H"], c["W"], c["C"], c["S"], c["L"]
    e8 = dt(0 if mutant == "no_eps" else 1e-8)
    w = inp["masks"].astype(dt)[:, :, pool_src(W, L, mutant)]           # [B, S, W]
    x = np.nan_to_num(inp["img"].astype(dt)) if inp["active"] is not None else inp["img"].astype(dt)
    out = np.zeros((B, S, 2, C, H), dt)
    with np.errstate(all="ignore"):
        for s in range(S):
            ws = w[:, s][:, None, :, None]                              # [B, 1, W, 1]
            v1 = ssum(w[:, s], 1)[:, None, None] + e8
            v2 = ssum(w[:, s] ** 2, 1)[:, None, None]
            mean = ssum(x * ws, 2) / v1                                 # [B, H, C]
            sq = ssum((x - mean[:, :, None]) ** 2 * ws, 2)
            var = sq / (v1 if mutant == "div_v1" else (v1 - v2 / v1 + e8))
            out[:, s, 0] = np.transpose(mean, (0, 2, 1))
            out[:, s, 1] = np.transpose(np.sqrt(var), (0, 2, 1))
    return dict(stats=out.reshape(B, S, 2 * C * H))


def pool_bound(c, inp, s=1.0):
    B, H, W, C, S, L = c["B"], c["H"], c["W"], c["C"], c["S"], c["L"]
    w = inp["masks"].astype(F64)[:, :, pool_src(W, L)]
    x = np.nan_to_num(inp["img"].astype(F64))
    out = np.zeros((B, S, 2, C, H))
    k = (W + 8) * s * U
    with np.errstate(all="ignore"):
        for s in range(S):
            ws = w[:, s][:, None, :, None]
            v1 = w[:, s].sum(1)[:, None, None] + 1e-8
            v2 = (w[:, s] ** 2).sum(1)[:, None, None]
            dv1 = k * v1
            mean = (x * ws).sum(2) / v1
            dmean = (k * (np.abs(x) * ws).sum(2) + np.abs(mean) * dv1) / v1 + U * np.abs(mean)
            d = np.abs(x - mean[:, :, None])
            ed = dmean[:, :, None] + U * d
            N = (d * d * ws).sum(2)
            dN = ((2 * d * ed + ed * ed + 3 * U * d * d) * ws).sum(2) + k * N
            D = v1 - v2 / v1 + 1e-8
            dD = dv1 + (v2 / v1) * (k + 2 * U + dv1 / v1) + U * np.abs(v1 - v2 / v1) + U * D
            lo = np.maximum(N - dN, 0) / (D + dD)
            hi = np.where(D - dD > 0, (N + dN) / np.where(D - dD > 0, D - dD, 1), np.inf)
            std = np.sqrt(N / D)
            bstd = np.maximum(np.sqrt(hi) * (1 + 4 * U) - std, std - np.sqrt(lo) * (1 - 4 * U))
            out[:, s, 0] = np.transpose(dmean, (0, 2, 1))
            out[:, s, 1] = np.transpose(np.broadcast_to(bstd, mean.shape), (0, 2, 1))
    if inp["active"] is not None:
        out[inp["active"] == 0] = 0.0                        # written as zeros, exactly
    return dict(stats=out.reshape(B, S, 2 * C * H))


# ---- window_active, compact_active ----------------------------------------------------------------------------------------
ACTIVE_B = (1, 255, 256, 257, 600)
ACTIVE_KINDS = ("none", "all", "third")


def active_flags(B, kind):
    f = np.zeros(B, np.int32)
    if kind == "all":
        f[:] = 1
    elif kind == "third":
        f[::3] = 1
    return f


# ---- comparison helpers ---------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound, an element being worth inf when it is not finite while its bound is (a
    finite, non-negative result is all an infinite bound asks for), 0 when it matches exactly"""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    r = np.where(np.isinf(bound) & np.isfinite(got) & (got >= 0), 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0
