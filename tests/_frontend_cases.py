"""Shared by test_frontend_kernels_gpu.py (device) and test_frontend_kernels_host.py (CPU): case tables, inputs, float64 references
and per-element error bounds of the kernels at the front of every segmentation forward — conv0_kernel<CPL, LN> (csrc/frontend.hip),
conv01_ws_kernel and split_weights_h2_frag_kernel (csrc/frontend_fused.hip) and the host factorisation of conv0's tap covariance
(conv0_lnq_factor, csrc/engine.cpp).  numpy (+ torch.erf through _small_cases); nothing here touches a device.

The conventions are those of _small_cases.py: one `<k>_run(case, inp, dt, ssum, mutant)` per family (float64 + exact sum = the
reference; float32 + a sequential sum = an IDEAL fp32 kernel; `mutant` = a subtly wrong kernel), one `<k>_bound(case, inp, s)`,
DERIVED, never tuned; accumulation shares carry the factor s, single roundings enter at face value.  u = 2^-24.

lnq          wbar = mean_c w_c and Q = cov_c(w_c) in longdouble from the fp32 taps; F (Q = F^T F) from the eigen-decomposition in
             double.  Before the cast to fp32 |F^T F - Q| <= 1e-12 max|Q| (the project's double-precision bar); the fp32 values the
             library ships are held to that + 2 u (1 + u) (|F|^T |F|)_ij, the rounding of the two factors of every product.
             lnq[0:10] == float32(wbar) bit for bit, entries of taps >= k exactly 0, C0 = 1: every entry finite and F == 0.

conv0        The reference is the model's statement: x = (wave - mean) rstd; y_c = sum_t w_ct x_t; mean and variance of y over the
             C0 real channels in two passes; erf-GELU of the affine.  With A_c = sum_t |w_ct x_t|:
               y      dy_c = 2 u A_c (the two roundings of x) + (10 + 8) s u A_c (the tap sum);
               lnq    mu = wbar . x with fp32 wbar: dmu = (1 + 2 + (10 + 8) s) u sum_j |wbar_j x_j|.  q_e = F_e . x with fp32 F:
                      dq_e = (1 + 2 + 11 s) u G_e, G_e = sum_j |F_ej x_j| (rounding of F, of x, the ten fmas and their start);
                      var = sum_e q_e^2: dvar = sum_e (2 |q_e| dq_e + dq_e^2) + (10 + 8) s u (var + that) + 1e-12 max|Q| (sum_j |x_j|)^2
                      (the factorisation's own bar);
               wave   mu = sum_c y_c / C0 from the computed outputs: dmu = mean_c dy_c + (C0 + 8) s u mean_c |y_c| + u |mu|;
                      d_c = y_c - mu: dd_c = dy_c + dmu + u |d_c|; M2 = sum d^2: dM2 = E + ((C0 + 8) s + 1) u (M2 + E),
                      E = sum_c (2 |d_c| dd_c + dd_c^2); dvar = dM2 / C0 + u var;
               rstd   1 / sqrt(var + eps): relative (1 - dvar / (var + eps))^-1/2 - 1 (infinite from dvar / (var + eps) >= 1/2:
                      no case reaches it) + u (the add) + 4 u (1 / sqrt at 2 ulp);
               pre    (y - mu) rstd gamma + beta: |rstd gamma| (dy + dmu + u |y - mu|) + |pre - beta| (drstd + 2 u) + u |pre|;
               GELU   1.13 dpre + 0.5 |pre| (ERF_ABS + 4 u) + 3 u |gelu(pre)|, as _small_cases.py.
             Raw mode (GroupNorm models): dy alone.  Columns [C0, Cp) are exactly 0.
             var_product_form (var as the plain fp32 sum x^T Q x) is what the factor F exists to avoid: on the stress case (taps
             whose rows sum to almost nothing, on a slow sine with a DC offset, so that x lies almost along Q's null directions)
             it leaves the bound: error / bound = 3.5 (test_frontend_kernels_host.py prints it), the ideal factor-form kernel 0.5.

split frag   exact: the bits of dzn_op_split_weights_h2 of the same W at [K/32][rows/16][2][16][32], every 32-block in natural k
             order (that kernel permutes k inside a block for its own fragment loads: H2_POS); the same col_scale.

conv01       float64 end to end: a = conv0 as above (lnq statistics; its taps summed as (even taps, odd taps, one add):
             phase_sum(2)), P[t, n] = sum_{j < 3} sum_c W[n, j C0 + c] a[2 t + j, c], then optionally LayerNorm over the C1 real
             channels and GELU.  With da the conv0 bound, K = 3 C0, S = sum |W| |a| and act_bound = fl(sqrt(C0)) max|gamma0| +
             max|beta0| as the engine computes it (every row's scale is the static bound):
               e = sum |W| da + (K + 8) s u S + 2^-21 S + 2^-38 act_bound sum_k |W|        (_gemm_cases.product_ref, "f32h")
             Epilogue LayerNorm: each of the two wavefronts of a row takes (mean, M2) of its 80 / C1 - 80 channels in two passes
             and the two are merged with Chan's update (four roundings): the `wave` statistics terms above with P for y, e for
             dy and C1 + 8 + 4 for C0 + 8.  amax1 is compared exactly with the maximum of the |out| the kernel stored (raw
             output: the tracker is not touched).
"""
from __future__ import annotations

import math

import numpy as np

from _small_cases import (ERF_ABS, GUARD, PATTERN, U, ULP_FN, EPS_LN, F32, F64, erf, exact_sum, gelu, phase_sum, seq_sum,   # noqa: F401
                          worst_ratio)

LNQ_BAR = 1e-12
TILE = 127                      # conv1 frames per (window, tile) item of conv01_ws_kernel


def _seed(name, i):
    return np.random.default_rng([sum(map(ord, name)), i])


# ---- lnq ------------------------------------------------------------------------------------------------------------------
LNQ_CASES = [dict(i=i, C0=C0, k=k) for i, (C0, k) in enumerate(((512, 10), (128, 10), (100, 7), (5, 3), (1, 10)))]


def taps(g, C0, k):
    return (g.standard_normal((C0, k)) * (0.5 + g.random((C0, 1))) / math.sqrt(k) + 0.05 * g.standard_normal(k)).astype(F32)


def lnq_inputs(c):
    return dict(w=taps(_seed("lnq", c["i"]), c["C0"], c["k"]))


def lnq_moments(w):
    """(wbar [10], Q [10, 10]) in longdouble from the fp32 taps w [C0, k]; taps >= k are zero"""
    C0, k = w.shape
    wl = w.astype(np.longdouble)
    wb = wl.sum(0) / C0
    d = wl - wb
    Q = d.T @ d / C0
    wbar, Qf = np.zeros(10, np.longdouble), np.zeros((10, 10), np.longdouble)
    wbar[:k], Qf[:k, :k] = wb, Q
    return wbar, Qf


def lnq_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    """dict(lnq [110] in dt, wbar, Q (float64)): F from the symmetric eigen-decomposition, F[e] = sqrt(lambda_e) v_e"""
    k = c["k"]
    wbar, Q = lnq_moments(inp["w"])
    Q64 = Q.astype(F64)
    lam, V = np.linalg.eigh(Q64[:k, :k])
    F = np.zeros((10, 10))
    F[:k, :k] = np.sqrt(np.maximum(lam, 0.0))[:, None] * V.T
    assert np.abs(F.T @ F - Q64).max() <= LNQ_BAR * max(np.abs(Q64).max(), 1e-300) or not Q64.any(), "the reference factor misses its own bar"
    return dict(lnq=np.concatenate([wbar.astype(F64), F.reshape(-1)]).astype(dt), wbar=wbar.astype(F64), Q=Q64)


def lnq_check(c, inp, lnq):
    """what a shipped lnq [110] float32 must satisfy (module docstring); raises AssertionError"""
    k, C0 = c["k"], c["C0"]
    ref = lnq_run(c, inp)
    lnq = np.asarray(lnq)
    assert lnq.dtype == F32 and lnq.shape == (110,) and np.isfinite(lnq).all(), f"lnq is not 110 finite floats: {c}"
    assert np.array_equal(lnq[:10].view(np.uint32), ref["wbar"].astype(F32).view(np.uint32)), f"lnq[0:10] is not float32(wbar): {c}"
    F = lnq[10:].reshape(10, 10).astype(F64)
    assert not F[:, k:].any() and not lnq[k:10].any(), f"entries of unused taps are not zero: {c}"
    Q = ref["Q"]
    tol = LNQ_BAR * np.abs(Q).max() + 2 * U * (1 + U) * (np.abs(F).T @ np.abs(F))
    assert (np.abs(F.T @ F - Q) <= tol).all(), f"F^T F misses Q by {np.abs(F.T @ F - Q).max():.3e} (max|Q| {np.abs(Q).max():.3e}): {c}"
    if C0 == 1:
        assert not F.any(), f"one channel has no variance, F must be zero: {c}"


# ---- conv0 ----------------------------------------------------------------------------------------------------------------
WIDTHS = ((512, 512), (256, 256), (260, 288), (100, 128), (5, 32), (1, 32))
T0S = (1, 3, 4, 5, 63, 64, 65, 129)
KS = ((10, 5), (10, 8), (7, 3), (1, 1))
MODES = ("lnq", "wave", "raw")
C0_MUTANTS = ("frame_shift", "block_edge", "stats_neighbour", "eps_outside", "unbiased_var", "stats_over_padded", "wstats_window0",
              "var_product_form")


def c0_cpl(C0, Cp):
    """launch_conv0's choice of channels per lane"""
    return 4 if max(C0, Cp) <= 256 else 8


def c0_cases():
    out = []

    def add(C0, Cp, T0, k, s, mode, stats, stress=False):
        i = len(out)
        out.append(dict(i=i, B=3, C0=C0, Cp=Cp, T0=T0, k=k, s=s, mode=mode, stats=stats, stress=stress, N=(T0 - 1) * s + k + i % 5))

    n = 0
    for C0, Cp in WIDTHS:                                   # every width in every mode
        for mode in MODES:
            k, s = KS[n % 4]
            add(C0, Cp, T0S[(3 * n + 1) % 8], k, s, mode, bool(n & 1))
            n += 1
    for C0, Cp in ((512, 512), (100, 128)):                 # both instantiations at every frame count
        for T0 in T0S:
            add(C0, Cp, T0, 10, 5, MODES[n % 3], bool((n >> 1) & 1))
            n += 1
    for k, s in KS:                                         # every tap count / stride with a full 64-frame block and a tail
        for mode in ("lnq", "wave"):
            add(260, 288, 65, k, s, mode, bool(n & 1))
            n += 1
    add(512, 512, 65, 10, 5, "lnq", False, stress=True)
    add(512, 512, 65, 10, 5, "wave", False, stress=True)
    return out


def _waves(g, B, N, stress):
    t = np.arange(N)
    if stress:                                              # a slow sine on a DC offset: ten samples are almost a constant
        w0 = 0.5 + 0.3 * np.sin(2 * np.pi * t / 4000.0 + 0.4)
        return np.stack([w0, 1e-4 * w0, 40.0 * w0])[:B].astype(F32)
    w0 = (0.05 * np.sin(2 * np.pi * t / 73.0) + 0.03 * np.sin(2 * np.pi * t / 11.3 + 1.0) + 0.02 * g.standard_normal(N) + 0.004)
    w = np.stack([w0 * sc for sc in (1.0, 1e-4, 40.0)])     # as recorded; so quiet that var << eps; loud
    if B > 3:
        w = np.concatenate([w, 0.1 * g.standard_normal((B - 3, N)) * (0.2 + g.random((B - 3, 1)))])
    return w[:B].astype(F32)


def _wave_stats(wave):
    w = wave.astype(F64)
    return np.stack([w.mean(1), 1.0 / np.sqrt(w.var(1) + EPS_LN)], 1).astype(F32)


def c0_inputs(c):
    g = _seed("c0", c["i"])
    C0, k = c["C0"], c["k"]
    if c["stress"]:                                         # rows that sum to almost nothing: DC-blocking / band-pass taps
        w = g.standard_normal((C0, k)) / math.sqrt(k)
        w = w - w.mean(1, keepdims=True) + 1e-4 * g.standard_normal((C0, 1)) + 0.3 * np.hanning(k + 2)[1:-1] / k
        w = w.astype(F32)
    else:
        w = taps(g, C0, k)
    wave = _waves(g, c["B"], c["N"], c["stress"])
    inp = dict(wave=wave, w=w, stats=_wave_stats(wave) if c["stats"] else None,
               gamma=(1 + 0.3 * g.standard_normal(C0)).astype(F32), beta=(0.3 * g.standard_normal(C0)).astype(F32))
    r = lnq_run(dict(k=k), inp)
    inp.update(lnq=r["lnq"].astype(F32), wbar=r["wbar"], Q=r["Q"], F=r["lnq"][10:].reshape(10, 10))
    return inp


def _x(c, inp, dt, mutant=None):
    wave = inp["wave"].astype(dt)
    if inp["stats"] is None:
        return wave
    st = inp["stats"].astype(dt)
    if mutant == "wstats_window0":
        st = np.broadcast_to(st[:1], st.shape)
    return ((wave - st[:, :1]) * st[:, 1:2]).astype(dt)


def _frames(x, T0, k, s, mutant=None):
    """x [B, N] -> X [B, T0, 10]: the k samples of every frame, taps >= k zero"""
    f = np.arange(T0)
    org = f * s + (1 if mutant == "frame_shift" else 0)
    if mutant == "block_edge":
        org = np.where(f >= 64, (f - 64) * s, org)
    xp = np.concatenate([x, np.zeros((x.shape[0], 1), x.dtype)], 1)
    X = np.zeros((x.shape[0], T0, 10), x.dtype)
    X[..., :k] = xp[:, org[:, None] + np.arange(k)[None]]
    return X


def _taps10(w, dt):
    out = np.zeros((w.shape[0], 10), dt)
    out[:, :w.shape[1]] = w
    return out


def conv0_ln(c, inp, dt, ssum, mutant, mode, C0=None, Cp=None):
    """y, then (LayerNorm + GELU unless mode == 'raw') -> [B, T0, C0] in dt"""
    C0 = C0 or c["C0"]
    k, s, T0 = c["k"], c["s"], c["T0"]
    X = _frames(_x(c, inp, dt, mutant), T0, k, s, mutant)
    w = _taps10(inp["w"], dt)
    if ssum is exact_sum:
        y = X @ w.T
    else:
        y = ssum((X[:, :, None, :] * w[None, None]).astype(dt), 3)
    if mode == "raw":
        return y
    one = dt(1)
    if mutant == "var_product_form":
        X32, Q32 = X.astype(F32), inp["Q"].astype(F32)
        var = seq_sum((X32[..., :, None] * Q32 * X32[..., None, :]).reshape(X.shape[:2] + (100,)), 2).astype(dt)[..., None]
        mu = (ssum(y, 2) / dt(C0))[..., None]
    elif mode == "lnq" and dt is F32:                       # the ideal kernel of the lnq path takes its statistics from the samples
        lq = inp["lnq"]
        mu = ssum(X * lq[:10], 2)[..., None]
        q = ssum((X[:, :, None, :] * lq[10:].reshape(10, 10)[None, None]).astype(dt), 3)
        var = ssum(q * q, 2)[..., None]
    else:
        div = dt(Cp or c["Cp"]) if mutant == "stats_over_padded" else dt(C0)
        mu = (ssum(y, 2) / div)[..., None]
        d = y - mu
        m2 = ssum(d * d, 2) + (dt((Cp or c["Cp"]) - C0) * mu[..., 0] ** 2 if mutant == "stats_over_padded" else dt(0))
        var = (m2 / (dt(max(C0 - 1, 1)) if mutant == "unbiased_var" else div))[..., None]
    eps = dt(EPS_LN)
    rs = one / (np.sqrt(var) + eps) if mutant == "eps_outside" else one / np.sqrt(var + eps)
    if mutant == "stats_neighbour":
        nb = np.minimum(np.arange(T0) ^ 1, T0 - 1)
        mu, rs = mu[:, nb], rs[:, nb]
    pre = (y - mu) * rs * inp["gamma"].astype(dt) + inp["beta"].astype(dt)
    return gelu(pre.astype(dt))


def c0_run(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    out = np.zeros((c["B"], c["T0"], c["Cp"]), dt)
    out[..., :c["C0"]] = conv0_ln(c, inp, dt, ssum, mutant, c["mode"])
    return dict(out=out)


def _rstd_rel(dvar, ve):
    r = dvar / ve
    with np.errstate(all="ignore"):
        return np.where(r < 0.5, (1 - np.minimum(r, 0.5)) ** -0.5 - 1, np.inf) + U + ULP_FN


def ln_gelu_bound(y, dy, gamma, beta, K, s, stats=None):
    """bound of gelu(LN(y) gamma + beta) over the last axis; y exact, dy its bound.  stats None: (mean, M2) from the computed
    values with K s u accumulation shares; else (dmu, dvar) of statistics that came from elsewhere"""
    C = y.shape[-1]
    mu = y.mean(-1, keepdims=True)
    d = y - mu
    var = (d * d).mean(-1, keepdims=True)
    if stats is None:
        dmu = dy.mean(-1, keepdims=True) + K * s * U * np.abs(y).mean(-1, keepdims=True) + U * np.abs(mu)
        dd = dy + dmu + U * np.abs(d)
        E = (2 * np.abs(d) * dd + dd * dd).sum(-1, keepdims=True)
        dvar = (E + (K * s + 1) * U * (C * var + E)) / C + U * var
    else:
        dmu, dvar = stats
    ve = var + EPS_LN
    rs = 1 / np.sqrt(ve)
    n = d * rs * gamma
    pre = n + beta
    dpre = np.abs(rs * gamma) * (dy + dmu + U * np.abs(d)) + np.abs(n) * (_rstd_rel(dvar, ve) + 2 * U) + U * np.abs(pre)
    return 1.13 * dpre + 0.5 * np.abs(pre) * (ERF_ABS + 4 * U) + 3 * U * np.abs(gelu(pre))


def lnq_stats_bound(X, inp, s):
    """(dmu, dvar) [B, T0, 1] of the statistics the lnq path takes from the samples X [B, T0, 10] (float64)"""
    aX = np.abs(X)
    dmu = (3 + 18 * s) * U * (aX @ np.abs(inp["wbar"]))
    F = inp["F"]
    q, G = X @ F.T, aX @ np.abs(F).T
    dq = (3 + 11 * s) * U * G
    E = (2 * np.abs(q) * dq + dq * dq).sum(-1)
    dvar = E + 18 * s * U * ((q * q).sum(-1) + E) + LNQ_BAR * np.abs(inp["Q"]).max() * aX.sum(-1) ** 2
    return dmu[..., None], dvar[..., None]


def conv0_bound(c, inp, mode, s, C0=None):
    """(y or the activation a [B, T0, C0] in float64, its bound)"""
    C0 = C0 or c["C0"]
    X = _frames(_x(c, inp, F64), c["T0"], c["k"], c["s"])
    w = _taps10(inp["w"], F64)
    y = X @ w.T
    dy = (2 + 18 * s) * U * (np.abs(X) @ np.abs(w).T)
    if mode == "raw":
        return y, dy
    gam, bet = inp["gamma"].astype(F64), inp["beta"].astype(F64)
    st = lnq_stats_bound(X, inp, s) if mode == "lnq" else None
    return conv0_ln(c, inp, F64, exact_sum, None, mode, C0), ln_gelu_bound(y, dy, gam, bet, C0 + 8, s, st)


def c0_bound(c, inp, s=1.0):
    b = np.zeros((c["B"], c["T0"], c["Cp"]))
    b[..., :c["C0"]] = conv0_bound(c, inp, c["mode"], s)[1]
    return dict(out=b)


# ---- split_weights_h2_frag ------------------------------------------------------------------------------------------------
FRAG_SHAPES = ((160, 384), (160, 1536), (16, 32))


def frag_inputs(rows, K):
    g = _seed("frag", rows + K)
    W = (g.standard_normal((rows, K)) * np.exp2(g.integers(-12, 6, (rows, 1)))).astype(F32)
    W[rows // 2] = 0.0                                      # scale 1, zeros
    W[rows - 1] = np.clip(W[rows - 1], -0.9, 0.9)
    W[rows - 1, K // 3] = -1.0                              # the row's maximum is an exact power of two
    return W


def h2_split(W):
    """numpy statement of the two-term fp16 split: (planes uint16 [rows, K/32, 2, 32], col_scale f32 [rows])"""
    rows, K = W.shape
    m = np.abs(W).max(1)
    e = np.where(m > 0, np.floor(np.log2(np.where(m > 0, m, 1.0).astype(F64))), 14.0)
    sc, inv = np.exp2(14.0 - e).astype(F32), np.exp2(e - 14.0).astype(F32)
    x = W * sc[:, None]
    h = x.astype(np.float16)
    l = (x - h.astype(F32)).astype(np.float16)
    return np.stack([h.view(np.uint16).reshape(rows, K // 32, 32), l.view(np.uint16).reshape(rows, K // 32, 32)], 2), inv


H2_POS = [8 * ((kk & 15) >> 2) + (kk & 3) + 4 * (kk >> 4) for kk in range(32)]      # where split_weights_h2_kernel puts k % 32 in its block


def h2_natural(planes):
    """planes of dzn_op_split_weights_h2 [rows, K/32, 2, 32] with every 32-block back in natural k order"""
    return planes[..., H2_POS]


def frag_reindex(planes):
    """[rows, K/32, 2, 32] -> [K/32, rows/16, 2, 16, 32]"""
    rows, kb = planes.shape[:2]
    return np.ascontiguousarray(planes.reshape(rows // 16, 16, kb, 2, 32).transpose(2, 0, 3, 1, 4))


# ---- conv01 ---------------------------------------------------------------------------------------------------------------
C01_MUTANTS = ("drop_cross_term", "tile_seam", "stale_row_stats", "merge_counts", "last_frame_zero", "tap_channel_order",
               "wstats_window0", "scale_of_tracker")
C01_T1 = (1, 126, 127, 128, 254, 255)
N1P = 160


def c01_cases(P):
    """P: workgroups the launcher starts at most (the device's multi_processor_count); the last two cases walk the persistent loop"""
    out = []

    def add(B, C0, C1, T1, extra, ln, amax, wstats):
        i = len(out)
        T0 = 2 * T1 + 1 + extra
        out.append(dict(i=i, B=B, C0=C0, C1=C1, T1=T1, T0=T0, ln=ln, amax=amax, wstats=wstats, N=(T0 - 1) * 5 + 10 + i % 5, P=P,
                        k=10, s=5, stats=wstats))

    n = 0
    for T1 in C01_T1:                                       # every tile edge with both parities of T0
        for extra in (0, 1):
            add(3, (128, 192, 512)[n % 3], (81, 153, 160)[(n // 2) % 3], T1, extra, bool(n & 1), ("none", "zero", "high")[(n // 2) % 3],
                bool((n >> 1) & 1))
            n += 1
    for C0 in (128, 192, 512):                              # every width pair through the epilogue LayerNorm
        for C1 in (81, 153, 160):
            add(3, C0, C1, 3, n & 1, True, ("zero", "high", "none")[n % 3], bool(n & 1))
            n += 1
    add(2 * P + 1, 128, 153, 3, 0, True, "zero", True)      # workgroup 0 walks three items, the others two
    add(P + 1, 128, 81, 128, 1, True, "zero", False)        # two tiles per window: consecutive items of a workgroup change window
    add(P + 1, 128, 160, 128, 0, False, "none", True)
    return out


def act_bound(inp, C0):
    """sqrt(C0) max|gamma0| + max|beta0| in fp32, as the engine computes it"""
    return float(F32(np.sqrt(F32(C0))) * np.abs(inp["gamma"]).max() + np.abs(inp["beta"]).max())


def c01_inputs(c):
    g = _seed("c01", c["i"])
    B, C0, C1 = c["B"], c["C0"], c["C1"]
    wave = _waves(g, B, c["N"], False)
    W = np.zeros((N1P, 3 * C0), F32)                        # [n][j C0 + c], zero rows n >= C1
    W[:C1] = g.standard_normal((C1, 3 * C0)) * (0.5 + g.random((C1, 1))) / math.sqrt(3 * C0)
    inp = dict(wave=wave, w=taps(g, C0, 10), stats=_wave_stats(wave) if c["wstats"] else None,
               gamma=(1 + 0.3 * g.standard_normal(C0)).astype(F32), beta=(0.3 * g.standard_normal(C0)).astype(F32), W=W,
               gamma1=(1 + 0.3 * g.standard_normal(C1)).astype(F32), beta1=(0.3 * g.standard_normal(C1)).astype(F32))
    r = lnq_run(dict(k=10), inp)
    inp.update(lnq=r["lnq"].astype(F32), wbar=r["wbar"], Q=r["Q"], F=r["lnq"][10:].reshape(10, 10), act_bound=act_bound(inp, C0))
    return inp


def _pow2_h2(m):
    """the exact power of two that puts m into [2^14, 2^15)"""
    return np.exp2(14.0 - np.floor(np.log2(m)))


def _h2(x, scale):
    xs = (x.astype(F64) * scale).astype(F32)
    h = xs.astype(np.float16).astype(F32)
    l = (xs - h).astype(np.float16).astype(F32)
    return h.astype(F64) / scale, l.astype(F64) / scale


def _a2(a, T1, mutant=None, C0=None):
    """a [B, T0, C0] -> the A operand of conv1 [B, T1, 3 C0]: K = (tap, channel)"""
    T0 = a.shape[1]
    t = np.arange(T1)
    org = 2 * t
    if mutant == "tile_seam":
        org = 2 * (t // TILE) * 128 + 2 * (t % TILE)
    fr = [np.minimum(org + j, T0 - 1) for j in range(3)]
    A = np.stack([a[:, f] for f in fr], 2)                  # [B, T1, 3, C0]
    if mutant == "tap_channel_order":
        A = A.transpose(0, 1, 3, 2)
    return A.reshape(a.shape[0], T1, -1)


def c01_korder(C0, kernel):
    """the order in which the K = 3 C0 products of an output are added, in 32-blocks: natural, or the kernel's (slab, tap, half)"""
    if not kernel:
        return [32 * i for i in range(3 * C0 // 32)]
    return [j * C0 + 32 * (2 * sl + kb) for sl in range(C0 // 64) for j in range(3) for kb in range(2)]


def a01(c, inp, dt=F64, ssum=exact_sum, mutant=None):
    return conv0_ln(c, inp, dt, ssum, mutant if mutant == "wstats_window0" else None, "lnq", c["C0"], c["C0"])


def c01_run(c, inp, dt=F64, ssum=exact_sum, mutant=None, kernel_order=False, a=None):
    """a: conv0's activations [B, T0, C0] from elsewhere (the unfused kernel's) instead of their reference"""
    B, C0, C1, T1, T0 = c["B"], c["C0"], c["C1"], c["T1"], c["T0"]
    a = a01(c, inp, dt, ssum, mutant) if a is None else a.astype(dt)
    if mutant == "last_frame_zero":
        a = a.copy()
        a[:, T0 - 1] = 0
    A = _a2(a, T1, mutant).reshape(B * T1, 3 * C0)
    W = inp["W"]
    if dt is F64 and mutant not in ("drop_cross_term", "scale_of_tracker"):
        P = A @ W.astype(F64).T
    else:                                                   # the two-term fp16 arithmetic: lo hi, hi lo, hi hi
        sa = _pow2_h2(inp["act_bound"])
        if mutant == "scale_of_tracker":
            sa = _pow2_h2(np.maximum(np.abs(A).max(1, keepdims=True), 1e-30))
        ah, al = _h2(A.astype(F32), sa)
        wh, wl = _h2(W, _pow2_h2(np.maximum(np.abs(W).max(1, keepdims=True), 1e-30)))
        terms = [(ah, wl), (ah, wh)] if mutant == "drop_cross_term" else [(al, wh), (ah, wl), (ah, wh)]
        if dt is F64:
            P = sum(x @ y.T for x, y in terms)
            if mutant == "scale_of_tracker":
                P = P * (sa / _pow2_h2(inp["act_bound"]))
        else:
            P = np.zeros((B * T1, N1P), F32)
            for k0 in c01_korder(C0, kernel_order):
                for x, y in terms:
                    P = P + x[:, k0:k0 + 32].astype(F32) @ y[:, k0:k0 + 32].astype(F32).T
    P = P.reshape(B, T1, N1P).astype(dt)
    if not c["ln"]:
        return dict(out=P)
    y = P[..., :C1]
    if dt is F32 or mutant in ("stale_row_stats", "merge_counts"):      # the two shares and their merge
        n0, n1 = dt(80), dt(C1 - 80)
        m0 = ssum(y[..., :80], 2) / n0
        m1 = ssum(y[..., 80:], 2) / n1
        q0 = ssum((y[..., :80] - m0[..., None]) ** 2, 2)
        q1 = ssum((y[..., 80:] - m1[..., None]) ** 2, 2)
        if mutant == "stale_row_stats":                     # the sibling's share of the item this workgroup finished before
            ntile = -(-T1 // TILE)
            grid = min(B * ntile, c["P"])
            b, t = np.meshgrid(np.arange(B), np.arange(T1), indexing="ij")
            item = b * ntile + t // TILE
            prev = item - grid
            pb, pt = prev // ntile, (prev % ntile) * TILE + t % TILE
            ok = (prev >= 0) & (pt < T1)
            pb, pt = np.where(ok, pb, b), np.where(ok, pt, t)
            m1, q1 = m1[pb, pt], q1[pb, pt]
        if mutant == "merge_counts" and C1 != 160:
            n1 = dt(80)
        n = n0 + n1
        dl = m1 - m0
        mu = (m0 + dl * (n1 / n))[..., None]
        var = ((q0 + q1 + dl * dl * (n0 * n1 / n)) / n)[..., None]
    else:
        mu = (ssum(y, 2) / dt(C1))[..., None]
        var = (ssum((y - mu) ** 2, 2) / dt(C1))[..., None]
    pre = (y - mu) * (dt(1) / np.sqrt(var + dt(EPS_LN))) * inp["gamma1"].astype(dt) + inp["beta1"].astype(dt)
    out = np.zeros((B, T1, N1P), dt)
    out[..., :C1] = gelu(pre.astype(dt))
    return dict(out=out)


def c01_bound(c, inp, s=1.0):
    B, C0, C1, T1 = c["B"], c["C0"], c["C1"], c["T1"]
    a, da = conv0_bound(c, inp, "lnq", s, C0)
    A, dA = _a2(a, T1).reshape(B * T1, -1), _a2(da, T1).reshape(B * T1, -1)
    aW = np.abs(inp["W"].astype(F64))
    S = np.abs(A) @ aW.T
    K = 3 * C0
    e = dA @ aW.T + (K + 8) * s * U * S + 2.0 ** -21 * S + 2.0 ** -38 * inp["act_bound"] * aW.sum(1)[None]
    e = e.reshape(B, T1, N1P)
    if not c["ln"]:
        return dict(out=e)
    P = (A @ inp["W"].astype(F64).T).reshape(B, T1, N1P)[..., :C1]
    b = np.zeros((B, T1, N1P))
    b[..., :C1] = ln_gelu_bound(P, e[..., :C1], inp["gamma1"].astype(F64), inp["beta1"].astype(F64), C1 + 8 + 4, s)
    return dict(out=b)
