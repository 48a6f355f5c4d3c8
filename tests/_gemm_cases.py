"""Shared by test_gemm_tiles_gpu.py (device) and test_gemm_bounds_host.py (CPU): the tile table of the contraction families, the
edge shapes and feature sets of the kernel-level matrix, its inputs, the float64 reference of a launch and the per-element error
bound that goes with it.  torch only; nothing here touches a device.

The bound is DERIVED, never tuned.  u = 2^-24 (unit round-off of fp32), S = sum_k |a||w| (+ |bias| where the bias joins the
accumulator directly):

  raw product      f32 / f32s : (K + 8) u S        one rounding per accumulation step; the three dropped products of the bf16
                                                   split are each below 2^-24 relative
                   f32h       : the same + 2^-21 S (22 significant bits kept per operand)
                                         + 2^-38 unit_max sum_k |w|   (the floor of the lo term, split.h / test_f32h_grade_gpu.py)
                   f16 / mx   : (K + 8) u S_h against the float64 product of the ROUNDED operands (testkit/mx_emulation.py,
                                per scale unit with that unit's a_amax); S_h = S on the rounded operands
  epilogue         every fp32 add / multiply adds u |result|; a function multiplies the incoming bound by its largest slope
                   (GELU 1.13, swish 1.10, ReLU 1); GELU adds 0.5 |x| (1.5e-7 + 8 u): the absolute error of common.h's erf
                   polynomial and one u for each of the eight fp32 operations that evaluate it (all of its intermediates are
                   below 1.5 in magnitude) and 2 u |gelu(x)| for 1 + erf and the last product; swish adds 8 u |swish(x)|
                   (expf, add, divide, multiply); the folded LayerNorm maps e -> rstd (e + u |mu colsum| + u |p - mu colsum|)
                   + u |x|
  weighted sum     the two launches' bounds, |ws_w| e each, + u per multiply / add
"""
from __future__ import annotations

import math

import torch

from testkit import mx_emulation as emu

U = 2.0 ** -24
PATTERN = 0x7FA5C3C3            # what every output band holds: a NaN as fp32, so an element nobody stored is not finite
GUARD_ROWS = 256                # rows of band before and after every 2-D buffer
A_AMAX_GUARD = 2.0 ** 60        # guard entries of a_amax: a row scaled by it underflows to 0 and fails its bound
WS_W = (0.3, -1.2)

# family -> (precision, profiler tag, {tile name: (BM, BN, WGM, WGN)})
_SPLIT = {"128x64": (128, 64, 4, 1), "128x80": (128, 80, 4, 1), "128x32": (128, 32, 4, 1)}
FAMILIES = {
    "f32": (0, "f32", {"128x32": (128, 32, 4, 1), "256x32": (256, 32, 4, 1), "256x64": (256, 64, 4, 1), "128x64": (128, 64, 2, 2),
                       "64x64": (64, 64, 2, 2), "128x128": (128, 128, 2, 2)}),
    "f32s": (2, "f32s", dict(_SPLIT, **{"128x128": (128, 128, 2, 2)})),
    "f32h": (3, "f32h", dict(_SPLIT, **{"128x128w4": (128, 128, 4, 1)})),
    "f16": (4, "f16", dict(_SPLIT, **{"128x128w4": (128, 128, 4, 1), "256x128w8s3": (256, 128, 8, 1)})),
    "mx": (4, "mx", {"128x64": (128, 64, 4, 1), "128x128": (128, 128, 4, 1), "256x128": (256, 128, 8, 1)}),
    "f32s_pre": (2, "f32s_pre", {"256x128": (256, 128, 4, 2), "128x128": (128, 128, 2, 2), "128x64": (128, 64, 4, 1)}),
}
FAMILY_TILES = [(f, t) for f, (_, _, tiles) in FAMILIES.items() for t in tiles]
PLAIN_AUTO_WIDTHS = [(564, 192), (308, 160), (276, 96)]      # N -> the column tile launch_f32 picks at K = 544 (all 128 rows, 2 x 2)


# ---- the automatic tile rules, restated from launch_f32 / launch_gemm_split_np / launch_gemm_mx ----
def auto_tile_f32(N, K):
    if N <= 32:
        return 256, 32
    if N <= 64 or (K <= 512 and N % 64 == 0):
        return 128, 64
    best, best_cols = 128, 1 << 30
    for c in (192, 160, 128, 96):
        cols = (N + c - 1) // c * c
        if cols < best_cols:
            best, best_cols = c, cols
    return 128, best


def auto_tile_split(family, M, N, K, nz=1):
    if N <= 32:
        return 128, 32
    if N <= 64 or K <= 512:
        return 128, 64
    cols128, cols64 = (N + 127) // 128 * 128, (N + 63) // 64 * 64
    if ((M + 127) // 128) * (cols128 // 128) * max(nz, 1) < 448:
        return 128, 64
    if N % 80 == 0 and N < cols64 and N * 9 < cols128 * 8:
        return 128, 80
    if cols64 * 9 < cols128 * 8:
        return 128, 64
    return (256, 128) if family == "f16" else (128, 128)


def auto_tile_mx(M, N, nz=1):
    cols128 = (N + 127) // 128 * 128
    narrow = N <= 64 or ((M + 127) // 128) * (cols128 // 128) * max(nz, 1) < 448
    return (128, 64) if narrow else (128, 128)


def edge_shapes(BM, BN, mx=False):
    """name -> (M, N, K, odd strides)"""
    return {"E1": (BM + 17, 2 * BN - 12, 96, False), "E2": (BM + 17, 2 * BN - 13, 64 if mx else 96, True),
            "E3": (BM - 1, BN + 4, 544, False), "E4a": (1, 4, 32, False), "E4b": (5, 3, 64, True), "E4c": (17, 36, 32, False)}


# feature sets: what the epilogue is asked to do
FEATURES = {
    "F0": dict(),
    "F1": dict(act=1, alpha=0.5, R=True, post_relu=True),
    "F2": dict(act=2, ws=True),
    "F3": dict(ln=True, stats=True),
    "F4": dict(rowoff=True),
}


def n_units(M, unit, nz=1):
    return (M + unit - 1) // unit if unit > 0 else nz


def row_units(M, unit, nz=1):
    """[nz, M] scale unit of every row: m / unit, or the z index when unit <= 0"""
    if unit > 0:
        return (torch.arange(M) // unit)[None, :].expand(nz, M)
    return torch.arange(nz)[:, None].expand(nz, M)


def make_inputs(M, N, K, unit, nz=1, seed=0):
    """A [nz, M, K] in scale units of `unit` rows (unit <= 0: one per z) whose loudness cycles 2^-9, 1, 2^7 and whose elements stay
    inside 2^10 of the unit maximum (so every lo term of the fp16 split keeps its bits), a_amax = the exact unit maxima; W [N, K]
    with per-row scales 0.5 .. 1.5 (asymmetric: a transposed store cannot pass) and elements inside 2^10 of 1; bias, R ~ 2^-6 N(0, 1)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 13 * max(unit, 0) + nz)
    loud = torch.tensor([2.0 ** -9, 1.0, 2.0 ** 7])
    ru = row_units(M, unit, nz)
    mag = torch.exp2(-10.0 * torch.rand(nz, M, K, generator=g))
    sgn = torch.randint(0, 2, (nz, M, K), generator=g).float() * 2 - 1
    A = (mag * sgn * loud[ru % 3][..., None]).float()
    nu = n_units(M, unit, nz)
    a_amax = torch.zeros(nu)
    a_amax.scatter_reduce_(0, ru.reshape(-1), A.abs().amax(-1).reshape(-1), "amax")
    wm = torch.exp2(-10.0 * torch.rand(N, K, generator=g))
    ws = torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1
    W = (wm * ws * torch.linspace(0.5, 1.5, N)[:, None]).float()
    # bias and residual at 2^-6: comparable with the products of the quiet units (so that a quiet row is held to a bound of its own
    # size) and far below the loud ones (so that a row counted into the wrong unit moves that unit's tracker)
    bias = torch.randn(N, generator=g) * 2.0 ** -6
    R = torch.randn(nz, M, N, generator=g) * 2.0 ** -6
    return dict(A=A, a_amax=a_amax, W=W, bias=bias, R=R, row_amax=a_amax[ru][..., None])


def h2_row_scale(amax):
    return emu._pow2_scale_h2(amax)


def operand_terms(family, A, row_amax, W):
    """the operand products the family's kernel adds up, smallest first as the kernel orders them: [(a [M, K], w [N, K])] float64,
    in unscaled units.  A [M, K] fp32, row_amax [M, 1] = the a_amax entry of each row's unit."""
    if family == "f32":
        return [(A.double(), W.double())]
    if family in ("f32s", "f32s_pre"):
        ah, am, al = emu.bf16x3_terms(A)
        wh, wm, wl = emu.bf16x3_terms(W)
        return [(al, wh), (ah, wl), (am, wm), (am, wh), (ah, wm), (ah, wh)]
    w_amax = W.abs().amax(dim=1, keepdim=True)
    if family in ("f32h", "f16"):
        ah, al = emu.h2_terms(A, h2_row_scale(row_amax))
        wh, wl = emu.h2_terms(W, h2_row_scale(w_amax))
        return [(al, wh), (ah, wl), (ah, wh)] if family == "f32h" else [(ah, wh)]
    assert family == "mx"
    ah, ah8, al8 = emu.mx_operand_terms(A, row_amax)
    wh, wh8, wl8 = emu.mx_operand_terms(W, w_amax)
    return [(ah8, wl8), (al8, wh8), (ah, wh)]


def product_ref(family, A, row_amax, W, bias_abs=None):
    """(P, e, terms): the float64 value the family is held to (the exact product; for f16 / mx the product of the rounded
    operands), its per-element bound before any epilogue, and the operand terms.  bias_abs [N] joins S where the bias is added
    straight onto the accumulator."""
    K = A.shape[1]
    terms = operand_terms(family, A, row_amax, W)
    if family in ("f16", "mx"):
        P = sum(a @ w.T for a, w in terms)
        S = sum(a.abs() @ w.abs().T for a, w in terms)
    else:
        P = A.double() @ W.double().T
        S = A.double().abs() @ W.double().abs().T
    if bias_abs is not None:
        S = S + bias_abs.double()[None, :]
    e = (K + 8) * U * S
    if family == "f32h":
        e = e + 2.0 ** -21 * S + 2.0 ** -38 * row_amax.double() * W.double().abs().sum(1)[None, :]
    return P, e, terms


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def epilogue_ref(P, e, *, bias=None, ln=None, act=0, alpha=1.0, R=None, post_relu=False, bias_in_S=False):
    """float64 epilogue chain of gemm_epilogue.h on the product P with bound e -> (C, eC, eC_acc).  ln = (mu [M], rstd [M], colsum
    [N]) as the kernel reads them (fp32 values).  bias_in_S: e already covers the bias add ((K + 8) u |bias| inside S).
    eC_acc <= eC is the share of the bound that descends from the product bound (the accumulation, whose order a kernel is free to
    choose); the rest, r, is the epilogue's own single roundings and function approximations, which no kernel can exceed and
    which therefore need no room (test_gemm_bounds_host.py)."""
    x = P
    r = torch.zeros_like(P)
    if ln is not None:
        mu, rs, cs = (t.double() for t in ln)
        t = mu[:, None] * cs[None, :]
        d = x - t
        x = rs[:, None] * d
        e = rs[:, None].abs() * e
        r = rs[:, None].abs() * (r + U * t.abs() + U * d.abs()) + U * x.abs()
    if bias is not None:
        x = x + bias.double()[None, :]
        if not (bias_in_S and ln is None):
            r = r + U * x.abs()
    if act == 1:
        y = _gelu64(x)
        e, r = 1.13 * e, 1.13 * r + 0.5 * x.abs() * (1.5e-7 + 8 * U) + 2 * U * y.abs()
        x = y
    elif act == 2:
        y = x * torch.sigmoid(x)
        e, r = 1.10 * e, 1.10 * r + 8 * U * y.abs()
        x = y
    elif act == 3:
        x = torch.relu(x)
    a = float(torch.tensor(alpha, dtype=torch.float32))
    if a != 1.0:
        x = x * a
        e, r = abs(a) * e, abs(a) * r + U * x.abs()
    if R is not None:
        x = x + R.double()
        r = r + U * x.abs()
    if post_relu:
        x = torch.relu(x)
    return x, e + r, e


def ws_ref(C, eC, eC_acc):
    """the layer-weighted sum after ws_init = True, ws_w = 0.3 and then ws_init = False, ws_w = -1.2 on the same C"""
    w1, w2 = (float(torch.tensor(w, dtype=torch.float32)) for w in WS_W)
    s1 = w1 * C
    e1 = abs(w1) * eC + U * s1.abs()
    t = w2 * C
    s2 = s1 + t
    e2 = e1 + abs(w2) * eC + U * t.abs() + U * s2.abs()
    return s2, e2, (abs(w1) + abs(w2)) * eC_acc


def launch_ref(family, inp, z, feat, ln=None):
    """reference of one z slab of a launch with feature set `feat` (a FEATURES value): dict(C, eC, eC_acc[, WS, eWS, eWS_acc])"""
    A, W = inp["A"][z], inp["W"]
    bias = inp["bias"]
    P, e, _ = product_ref(family, A, inp["row_amax"][z], W, None if feat.get("ln") else bias.abs())
    C, eC, eA = epilogue_ref(P, e, bias=bias, ln=ln, act=feat.get("act", 0), alpha=feat.get("alpha", 1.0),
                             R=inp["R"][z] if feat.get("R") else None, post_relu=feat.get("post_relu", False), bias_in_S=True)
    out = dict(C=C, eC=eC, eC_acc=eA)
    if feat.get("ws"):
        out["WS"], out["eWS"], out["eWS_acc"] = ws_ref(C, eC, eA)
    return out


# ---- an ideal kernel on the CPU: the family's operand rounding, fp32 accumulation in a stated order, an fp32 epilogue ----
def ideal_accumulate(terms, order):
    """fp32 accumulation of the operand products, one rounding per step.  "forward": k = 0 .. K-1, every term at each k;
    "blocked": 32-blocks of k, per block every term, per term the exact sum of 4 consecutive products rounded to fp32, then added"""
    M, K = terms[0][0].shape
    N = terms[0][1].shape[0]
    acc = torch.zeros(M, N, dtype=torch.float32)
    if order == "forward":
        for k in range(K):
            for a, w in terms:
                acc = (acc.double() + a[:, k:k + 1] * w[:, k][None, :]).float()
        return acc
    for k0 in range(0, K, 32):
        for a, w in terms:
            for k in range(k0, min(k0 + 32, K), 4):
                p = (a[:, k:k + 4] @ w[:, k:k + 4].T).float()
                acc = (acc.double() + p.double()).float()
    return acc


def ideal_epilogue(acc, *, bias=None, ln=None, act=0, alpha=1.0, R=None, post_relu=False):
    """gemm_epilogue.h's chain in fp32 torch arithmetic"""
    x = acc
    if ln is not None:
        mu, rs, cs = ln
        x = rs[:, None] * (x - mu[:, None] * cs[None, :])
    if bias is not None:
        x = x + bias[None, :]
    if act == 1:
        x = torch.nn.functional.gelu(x)
    elif act == 2:
        x = x * torch.sigmoid(x)
    x = x * torch.tensor(alpha, dtype=torch.float32)
    if R is not None:
        x = x + R
    if post_relu:
        x = torch.relu(x)
    return x


def host_ln(A, W, K, eps=1e-5):
    """(mu, rstd, colsum) fp32 as a folded LayerNorm would hand them over: row statistics of A, row sums of W"""
    mu = A.double().mean(1)
    var = A.double().var(1, unbiased=False)
    return mu.float(), (var + eps).rsqrt().float(), W.double().sum(1).float()
