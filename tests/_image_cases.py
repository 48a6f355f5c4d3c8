"""Shared by test_image_kernels_gpu.py (device) and test_image_kernels_host.py (CPU): case tables, inputs, float64 references and
per-element error bounds of the hand-scheduled image kernels of the embedding trunk — csrc/conv_split.hip
(conv3x3_c32_split_kernel<3 | 2>), csrc/resblock_fused.hip (resblock32_fused_kernel<2 | 1>) and csrc/resblock_ws.hip
(resblock_ws_kernel<32 | 64, 2 | 1>) — in the launch form the engine uses (dzn_op_*_ex: caller-owned output, |max| trackers,
device-chosen image lists, explicit number of terms).  numpy and torch on the CPU; nothing here touches a device.

Each kernel has ONE function `<k>_run(case, inp, dt, ssum, mutant)` that states the operation as wespeaker/resnet.py:139-144
defines it with BatchNorm folded, over zero-bordered NHWC images [B][H + 2][W + 2][C] and weights [C][k], k = (dh*3 + dw) * C + ci:

    conv   out = [relu]( conv(x) + b ) [+ R] [relu]
    block  out = relu( conv2( relu(conv1(x) + b1) ) + b2 + x )

With dt = float64 and no order it is the reference (exact operands, exact sum).  With dt = float32 and ssum = "forward" / "reverse"
it is an IDEAL fp32 kernel: the operands split as the kernel splits them (testkit/mx_emulation.py restates split.h; h2_scale below
restates its fallbacks), the products SplitTerms lists added in fp32 one rounding per step in that order, every epilogue operation
rounded once; the block's intermediate is split again at the scale of the a-priori bound amax_in * l1max1 + bmax1.  With `mutant` it
is one of the subtly wrong kernels test_image_kernels_host.py holds the bound against.

The bound is DERIVED, never tuned, with the accounting of _gemm_cases.py.  u = 2^-24, K = 9 C, S = sum |x||w| + |b|, s = the share
of the accumulation term that is granted (1 on the device; the host test shows an ideal kernel inside it at s = 1/4):

    per convolution   f32s (three bf16 terms): (K + 8) s u S
                      f32h (two fp16 terms)  : the same + 2^-21 S + 2^-38 unit_max sum |w|
                      unit_max = what h2_scale was handed: amax_in[b] for an input split (also a deliberately larger one),
                      amax_in[b] * l1max1 + bmax1 for the block's intermediate (the tracked |max| in the two-launch chain)
    epilogue          every fp32 operation adds u |result|; ReLU is 1-Lipschitz, so no element is ever left out
    block             e_out = sum |w2| e_mid + (conv2's own bound on the true intermediate) + u (|pre| + |pre + x|)
    np = 1            the fp16 rounding model against the float64 result on the UNROUNDED operands: every operand v carries
                      d_v = 2^-11 |v| + 2^-25 / scale (half a subnormal step), a product sum  sum (|x| d_w + |w| d_x + d_x d_w),
                      the intermediate its own error on top; carried through both convolutions.  Loose by nature: the geometry is
                      held by the two-term cases of the same templates and by the bit equalities of the device test.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import torch

from _small_cases import F32, F64, GUARD, PATTERN, U, worst_ratio  # noqa: F401  (re-exported for the two test files)
from testkit import mx_emulation as emu

STRIP = 60                       # output columns of a block item (resblock_fused.hip RB_OUT, resblock_ws.hip WS_OUT)
SLOTS = {32: 512, 64: 256}       # persistent workgroups of the block kernels per launch
CONV_GRID, CONV_TILE = 512, 128  # conv_split.hip: workgroups per launch (64 per XCD), flat padded pixels per tile
# (weight term, pixel term) of every product, smallest first: split.h SplitTerms<NP>::A / B (0 = hi)
PRODUCTS = {3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)), 2: ((1, 0), (0, 1), (0, 0)), 1: ((0, 0),)}
SPLIT_MUTANTS = ("neighbour_scale", "lo_dropped")     # wrong kernels that only exist on split operands
CONV_MUTANTS = ("row_wrap", "tap_transposed", "relu_after_residual_only", "neighbour_scale", "list_identity", "lo_dropped")
BLOCK_MUTANTS = ("mid_pad_live", "strip_seam", "tap_transposed", "neighbour_scale", "list_identity", "stale_ring", "lo_dropped")

EPILOGUES = (dict(relu=False, R=False, post=False), dict(relu=True, R=False, post=False), dict(relu=False, R=True, post=True),
             dict(relu=True, R=True, post=True))
TRACKERS = ("absent", "zero", "above", "below")
LISTS = ("none", "subset", "empty")


# ---- split.h, restated ----------------------------------------------------------------------------------------------------
def h2_scale(amax):
    """split.h h2_scale: the power of two that puts amax into [2^14, 2^15); amax <= 0 (an empty tracker), a NaN or an exponent
    above 100 give scale 1, exponents below -100 are clamped there"""
    a = np.ascontiguousarray(amax, F32)
    e = ((a.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    e = np.where(~(a > 0) | (e > 100), 14, e)
    return np.exp2(14.0 - np.maximum(e, -100))


def mid_unit(amax_in, l1max1, bmax1):
    """the a-priori bound of the intermediate as the kernels form it: fmaf(amax_in, l1max1, bmax1)"""
    return (np.asarray(amax_in, F64) * F64(F32(l1max1)) + F64(F32(bmax1))).astype(F32)


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32))


def pixel_terms(x, nterm, scale):
    """x [n, ...] -> the nterm operand terms (float64, unscaled units) of every image at its power-of-two scale [n]"""
    with np.errstate(all="ignore"):
        if nterm == 3:
            return [t.numpy() for t in emu.bf16x3_terms(_t32(x))]
        sc = torch.from_numpy(np.asarray(scale, F64).reshape((-1,) + (1,) * (x.ndim - 1)))
        return [t.numpy() for t in emu.h2_terms(_t32(x), sc)][:nterm]


def weight_scale(w):
    return emu._pow2_scale_h2(torch.from_numpy(np.abs(w).max(axis=1, keepdims=True).astype(F32))).numpy()


def weight_terms(w, nterm):
    """w [C, K] -> its terms, each row at the scale of its own |max| (dzn_op_split_weights / dzn_op_split_weights_h2)"""
    if nterm == 3:
        return [t.numpy() for t in emu.bf16x3_terms(_t32(w))]
    return [t.numpy() for t in emu.h2_terms(_t32(w), torch.from_numpy(weight_scale(w)))][:nterm]


# ---- the contraction --------------------------------------------------------------------------------------------------------
def patches(xp):
    """zero-bordered [n, H + 2, W + 2, C] -> [n, H, W, 9 C] with k = (dh*3 + dw) * C + ci"""
    H, W = xp.shape[1] - 2, xp.shape[2] - 2
    return np.concatenate([xp[:, dh:dh + H, dw:dw + W, :] for dh in range(3) for dw in range(3)], axis=-1)


def conv_exact(xp, w):
    """float64 sum_k patches(xp)[.., k] w[oc, k], image by image (memory)"""
    wt = np.asarray(w, F64).T
    return np.stack([patches(np.asarray(im, F64)[None])[0] @ wt for im in xp]) if len(xp) else np.zeros(
        (0, xp.shape[1] - 2, xp.shape[2] - 2, w.shape[0]))


def conv_terms(xts, wts, products, dt, order):
    """sum over the listed products of the operand terms: exact in float64, or in fp32 one rounding per step, k forward (every
    product at each k, smallest first) or all of it in reverse"""
    with np.errstate(all="ignore"):
        if dt is F64:
            return sum(conv_exact(xts[b], wts[a]) for a, b in products)
        n, H, W = xts[0].shape[0], xts[0].shape[1] - 2, xts[0].shape[2] - 2
        K, Co = 9 * xts[0].shape[3], wts[0].shape[0]
        # every term has at most 11 significant bits and the scales are powers of two: the fp32 product of two terms is exact
        px = [np.ascontiguousarray(patches(t).reshape(n * H * W, K).T, F32) for t in xts]
        wk = [np.ascontiguousarray(t.T, F32) for t in wts]
        steps = [(k, a, b) for k in range(K) for a, b in products]
        acc = np.zeros((n * H * W, Co), F32)
        for k, a, b in (steps if order == "forward" else steps[::-1]):
            acc = acc + px[b][k][:, None] * wk[a][k][None, :]
        return acc.reshape(n, H, W, Co)


def _pad(v):
    return np.pad(v, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _swap_taps(w):
    C = w.shape[0]
    return np.ascontiguousarray(w.reshape(C, 3, 3, -1).transpose(0, 2, 1, 3)).reshape(C, -1)


def _relu(v):
    return np.maximum(v, v.dtype.type(0))


# ---- cases --------------------------------------------------------------------------------------------------------------------
def case_images(c, mutant=None):
    """the images a launch works on, in list order"""
    if c["zl"] == "none":
        return list(range(c["B"]))
    sel = list(range(c["B"] - 1, -1, -2))        # a permuted proper subset: descending, every other image
    if c["zl"] == "empty":
        return []
    return list(range(len(sel))) if mutant == "list_identity" else sel


def list_buffers(c):
    """(z_count, z_list) int32 arrays as the launch gets them, or (None, None)"""
    if c["zl"] == "none":
        return None, None
    sel = np.asarray(range(c["B"] - 1, -1, -2), np.int32)
    return np.asarray([0 if c["zl"] == "empty" else sel.size], np.int32), sel


def _variants(n, B):
    zl = LISTS[n % 3]
    return dict(trk=TRACKERS[(n + n // 4) % 4], zl="none" if (B == 1 and zl == "subset") else zl, amax8=(n // 3) % 2 == 1)


CONV_SHAPES = ((1, 1), (1, 125), (1, 126), (1, 127), (2, 62), (3, 126), (5, 37), (12, 126), (66, 126))
CONV_B = (1, 3, 8, 9, 17)


@functools.lru_cache(maxsize=None)
def conv_cases():
    """shapes at the edges of the flat 128-pixel tiles (P = W + 2 = 64, 128, 129; npix < 128; tiles that start and end mid-row;
    66 tiles per image against 64 slots per XCD) x batch sizes around the 8 XCDs x both arithmetic forms, every other one kept;
    epilogue, tracker, list and the given amax_in cycle through the kept ones.  (66, 126) stays at B <= 9: 12 MB per buffer."""
    out = []
    for (i, (H, W)), (j, B), (k, nterm) in itertools.product(enumerate(CONV_SHAPES), enumerate(CONV_B), enumerate((3, 2))):
        if (i + j + k) % 2:
            continue
        n = len(out)
        B = min(B, 9) if H * W > 4096 else B
        v = _variants(n, B)
        if H * W > 4096 and B > 8:          # more tiles per image than an XCD has workgroups AND more images than XCDs: all of them
            v["zl"] = "none"
        out.append(dict(kernel="conv", i=n, C=32, H=H, W=W, B=B, np=nterm, l1x=1.0, **EPILOGUES[(n // 2) % 4], **v))
    return out


BLOCK_W = (1, 2, 59, 60, 61, 62, 63, 64, 120, 121)
BLOCK_H = (1, 2, 3, 4, 5, 6, 9)
BLOCK_B = (1, 3, 2, 4)


@functools.lru_cache(maxsize=None)
def block_cases(C):
    """strip widths x heights (the ring's `& 3` / `% 3` wrap), every other pair for C = 32 and the others for C = 64, both term
    counts each; then the launches with more items than workgroups (a workgroup runs a second item on rings the first one left)"""
    out = []
    for (i, W), (j, H) in itertools.product(enumerate(BLOCK_W), enumerate(BLOCK_H)):
        if (i + j) % 2 != (0 if C == 32 else 1):
            continue
        g = len(out) // 2
        B = BLOCK_B[g % 4]
        for nterm in (2, 1):
            out.append(dict(kernel="block", i=g, C=C, H=H, W=W, B=B, np=nterm, l1x=(1.0, 8.0)[(g // 2) % 2], **_variants(g, B)))
    g = len(out) // 2
    for nterm in (2, 1):
        out.append(dict(kernel="block", i=g, C=C, H=2, W=61, B=260 if C == 32 else 130, np=nterm, l1x=1.0, trk="zero", zl="none",
                        amax8=False))
    return out


def block_items(c):
    """(items of the launch, workgroups of the launch)"""
    nitem = len(case_images(c)) * -(-c["W"] // STRIP)
    return nitem, min(c["B"] * -(-c["W"] // STRIP), SLOTS[c["C"]])


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(C):
    """w1, w2 [C, 9 C]: magnitudes log-uniform inside 2^8 of 1 (every lo term of the fp16 split keeps its bits), both signs, row
    scales 0.5 .. 1.5 (a transposed store cannot pass), sized so that a layer keeps the loudness of its input; b1, b2 with both
    signs, |b| up to 0.5; l1max1 = max_oc sum_k |w1| (a hair above, as the engine's host code rounds it up), bmax1 = max |b1|"""
    g = np.random.default_rng([77, C])
    out = {}
    for name in ("w1", "w2"):
        mag = np.exp2(-8.0 * g.random((C, 9 * C)))
        sgn = g.integers(0, 2, (C, 9 * C)) * 2.0 - 1.0
        out[name] = (mag * sgn * np.linspace(0.5, 1.5, C)[:, None] * (0.25 * (32.0 / C) ** 0.5)).astype(F32)
    for name in ("b1", "b2"):
        out[name] = (g.uniform(0.05, 0.5, C) * (g.integers(0, 2, C) * 2.0 - 1.0)).astype(F32)
    out["b1"][:4] = (0.5, -0.5, 0.45, -0.3)
    out["l1max1"] = float(F32(np.abs(out["w1"]).astype(F64).sum(1).max() * (1 + 1e-6)))
    out["bmax1"] = float(np.abs(out["b1"]).max())
    return out


def loudness(B):
    """per image 2^+10, 2^-10, 2^+7, 2^-7, ...: a loud image next to a quiet one"""
    b = np.arange(B)
    return np.exp2(np.where(b % 2 == 0, 1.0, -1.0) * (10 - (3 * (b // 2)) % 11))


@functools.lru_cache(maxsize=6)
def _images(kernel, i, C, H, W, B):
    g = np.random.default_rng([sum(map(ord, kernel)), C, i, H, W, B])
    loud = loudness(B)[:, None, None, None]

    def image():
        v = np.exp2(-10.0 * g.random((B, H, W, C))) * (g.integers(0, 2, (B, H, W, C)) * 2.0 - 1.0) * loud
        if B >= 3:
            v[2] = 0.0                                         # an empty image: amax_in = 0, h2_scale falls back to scale 1
        return _pad(v).astype(F32)
    x = image()
    return x, (image() if kernel == "conv" else None)


def inputs(c):
    """x (and R for conv) zero-bordered fp32 [B, H + 2, W + 2, C]; amax_in [B] = the true per-image |max|, or 8 x it; weights"""
    x, R = _images(c["kernel"], c["i"], c["C"], c["H"], c["W"], c["B"])
    amax = np.abs(x).reshape(c["B"], -1).max(1).astype(F32) * F32(8.0 if c["amax8"] else 1.0)
    wt = weights(c["C"])
    return dict(x=x, R=R, amax_in=amax, l1max1=float(F32(wt["l1max1"] * c["l1x"])), **{k: wt[k] for k in ("w1", "w2", "b1", "b2", "bmax1")})


def _interior(xp):
    return xp[:, 1:-1, 1:-1, :]


# ---- conv -----------------------------------------------------------------------------------------------------------------------
def conv_run(c, inp, dt=F64, ssum=None, mutant=None, images=None):
    """-> dict(out [B, H, W, 32] in dt, NaN where the launch stores nothing).  images: work on these listed images only."""
    B, H, W, nterm = c["B"], c["H"], c["W"], c["np"]
    sel = [b for b in case_images(c, mutant) if images is None or b in images]
    x, w, bias = inp["x"][sel], inp["w1"], inp["b1"]
    if mutant == "row_wrap" and len(sel):         # the flat walk reads on across a row end: border columns hold the neighbours' pixels
        x = x.copy()
        x[:, :-1, W + 1] = inp["x"][sel][:, 1:, 1]
        x[:, 1:, 0] = inp["x"][sel][:, :-1, W]
    if mutant == "tap_transposed":
        w = _swap_taps(w)
    relu = c["relu"] and not (mutant == "relu_after_residual_only" and c["R"])
    if dt is F32 or mutant in SPLIT_MUTANTS:
        who = [(b + 1) % B for b in sel] if mutant == "neighbour_scale" else sel
        prods = PRODUCTS[nterm][1:] if (mutant == "lo_dropped" and nterm > 1) else PRODUCTS[nterm]
        acc = conv_terms(pixel_terms(x, nterm, h2_scale(inp["amax_in"][who])), weight_terms(w, nterm), prods, dt, ssum)
    else:
        acc = conv_exact(x, w)
    with np.errstate(all="ignore"):
        v = acc.astype(dt) + bias.astype(dt)
        if relu:
            v = _relu(v)
        if c["R"]:
            v = v + _interior(inp["R"][sel]).astype(dt)
        if c["post"]:
            v = _relu(v)
    out = np.full((B, H, W, 32), np.nan, dt)
    out[sel] = v
    return dict(out=out)


def _f32h_extra(S, unit_max, wabs_sum):
    return 2.0 ** -21 * S + 2.0 ** -38 * np.asarray(unit_max, F64)[:, None, None, None] * wabs_sum[None, None, None, :]


def conv_bound(c, inp, s=1.0):
    """per element [B, H, W, 32], every image"""
    x, w, bias = inp["x"].astype(F64), inp["w1"].astype(F64), inp["b1"].astype(F64)
    S = conv_exact(np.abs(x), np.abs(w)) + np.abs(bias)
    e = (w.shape[1] + 8) * s * U * S
    if c["np"] == 2:
        e = e + _f32h_extra(S, inp["amax_in"], np.abs(w).sum(1))
    v = conv_exact(x, w) + bias
    e = e + U * np.abs(v)
    if c["relu"]:
        v = _relu(v)
    if c["R"]:
        v = v + _interior(inp["R"]).astype(F64)
        e = e + U * np.abs(v)
    return dict(out=e)


# ---- BasicBlock -----------------------------------------------------------------------------------------------------------------
def block_run(c, inp, dt=F64, ssum=None, mutant=None, images=None, unit_mid=None):
    """-> dict(out [B, H, W, C] in dt, NaN where the launch stores nothing, mid [B, H, W, C] likewise).  unit_mid [B]: what the
    intermediate's split is scaled from instead of the a-priori bound (the two-launch chain: the tracked |max|)."""
    B, H, W, C, nterm = c["B"], c["H"], c["W"], c["C"], c["np"]
    sel = [b for b in case_images(c, mutant) if images is None or b in images]
    x, w1, w2 = inp["x"][sel], inp["w1"], inp["w2"]
    if mutant == "tap_transposed":
        w1, w2 = _swap_taps(w1), _swap_taps(w2)
    split = dt is F32 or mutant in SPLIT_MUTANTS
    who = [(b + 1) % B for b in sel] if mutant == "neighbour_scale" else sel
    prods = PRODUCTS[nterm][1:] if (mutant == "lo_dropped" and nterm > 1) else PRODUCTS[nterm]

    def conv(vp, w, scale):
        if split:
            return conv_terms(pixel_terms(vp, nterm, scale), weight_terms(w, nterm), prods, dt, ssum)
        return conv_exact(vp, w)
    with np.errstate(all="ignore"):
        live = mutant == "mid_pad_live"       # the intermediate outside the image is conv2's padding: zero, not relu(conv1 + b1)
        mid = _relu(conv(_pad(x) if live else x, w1, h2_scale(inp["amax_in"][who])).astype(dt) + inp["b1"].astype(dt))
        midp = mid if live else _pad(mid)
        um = mid_unit(inp["amax_in"], inp["l1max1"], inp["bmax1"]) if unit_mid is None else np.asarray(unit_mid, F32)
        acc = conv(midp.astype(F32) if split else midp, w2, h2_scale(um[who]))
        if mutant == "strip_seam":              # the first column of a strip from its left neighbour's last one
            for c0 in range(STRIP, W, STRIP):
                acc[:, :, c0] = acc[:, :, c0 - 1]
        if mutant == "stale_ring":              # a workgroup's second item: row -1 of the M ring still holds the first item's last row
            nstrip = -(-W // STRIP)
            nitem, grid = block_items(c)
            for item in range(grid, nitem):
                (bi, st), (pb, ps) = divmod(item, nstrip), divmod(item - grid, nstrip)
                if bi >= len(sel) or pb >= len(sel):
                    continue
                c0, p0 = st * STRIP, ps * STRIP
                loc = midp[bi:bi + 1, 0:3, c0:c0 + STRIP + 2].copy()
                old = midp[pb, H, p0:p0 + loc.shape[2]]
                loc[0, 0] = 0
                loc[0, 0, :old.shape[0]] = old
                acc[bi, 0, c0:c0 + loc.shape[2] - 2] = conv_exact(loc, w2)[0, 0]
        pre = acc.astype(dt) + inp["b2"].astype(dt)
        v = _relu(pre + _interior(x).astype(dt))
    out, m = np.full((B, H, W, C), np.nan, dt), np.full((B, H, W, C), np.nan, dt)
    out[sel] = v
    m[sel] = _interior(midp) if live else mid
    return dict(out=out, mid=m)


def block_bound(c, inp, s=1.0, unit_mid=None):
    """per element [B, H, W, C], every image: dict(out, mid)"""
    x, w1, w2 = inp["x"].astype(F64), inp["w1"].astype(F64), inp["w2"].astype(F64)
    b1, b2 = inp["b1"].astype(F64), inp["b2"].astype(F64)
    K = w1.shape[1]
    um = (mid_unit(inp["amax_in"], inp["l1max1"], inp["bmax1"]) if unit_mid is None else np.asarray(unit_mid, F32)).astype(F64)
    pre1 = conv_exact(x, w1) + b1
    mid = _relu(pre1)
    S1 = conv_exact(np.abs(x), np.abs(w1)) + np.abs(b1)
    S2 = conv_exact(_pad(mid), np.abs(w2)) + np.abs(b2)
    pre2 = conv_exact(_pad(mid), w2) + b2
    tail = U * np.abs(pre2) + U * np.abs(pre2 + _interior(x))
    if c["np"] == 2:
        e_mid = (K + 8) * s * U * S1 + _f32h_extra(S1, inp["amax_in"], np.abs(w1).sum(1)) + U * np.abs(pre1)
        e_out = conv_exact(_pad(e_mid), np.abs(w2)) + (K + 8) * s * U * S2 + _f32h_extra(S2, um, np.abs(w2).sum(1)) + tail
        return dict(out=e_out, mid=e_mid)
    bc = lambda v: np.asarray(v, F64)[:, None, None, None]
    dw1 = 2.0 ** -11 * np.abs(w1) + 2.0 ** -25 / weight_scale(inp["w1"])
    dw2 = 2.0 ** -11 * np.abs(w2) + 2.0 ** -25 / weight_scale(inp["w2"])
    dx = _pad(_interior(2.0 ** -11 * np.abs(x) + 2.0 ** -25 / bc(h2_scale(inp["amax_in"]))))
    e_mid = conv_exact(np.abs(x), dw1) + conv_exact(dx, np.abs(w1) + dw1) + (K + 8) * s * U * S1 + U * np.abs(pre1)
    dm = _pad(e_mid + 2.0 ** -11 * (mid + e_mid) + 2.0 ** -25 / bc(h2_scale(um)))
    e_out = conv_exact(_pad(mid), dw2) + conv_exact(dm, np.abs(w2) + dw2) + (K + 8) * s * U * S2 + tail
    return dict(out=e_out, mid=e_mid)


RUN = {"conv": conv_run, "block": block_run}
BOUND = {"conv": conv_bound, "block": block_bound}


# ---- trackers -------------------------------------------------------------------------------------------------------------------
def tracker_preload(c, ref_out):
    """amax_out [B] as the launch finds it: None (absent), zeros, above or below the result; images outside the list hold 3"""
    if c["trk"] == "absent":
        return None
    flat = np.abs(ref_out).reshape(c["B"], -1)
    m = np.where(np.isnan(flat).all(1), 3.0, np.max(np.nan_to_num(flat), axis=1))
    pre = {"zero": 0.0 * m, "above": 4.0 * m + 1.0, "below": 0.25 * m}[c["trk"]].astype(F32)
    out = np.full(c["B"], 3.0, F32)
    sel = case_images(c)
    out[sel] = pre[sel]
    return out


def tracker_after(c, preload, out):
    """what the tracker must hold after the launch stored `out` [B, H, W, C] (fp32 values): max(preload, max |out[b]|) bit for bit
    for the images of the list, the preload everywhere else; None when absent"""
    if preload is None:
        return None
    after = np.array(preload, F32)
    for b in case_images(c):
        after[b] = max(F32(preload[b]), np.abs(np.asarray(out[b], F32)).max())
    return after
