"""Thin torch-tensor wrappers over the kernel-level C ABI (include/dzn_ops.h).

Only used by tests/ and bench.py to exercise single kernels; the engine itself
orchestrates the same launchers in C++.  Tensors must live on the HIP device.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import DznGemmDesc, check


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gemm(A, W, *, M=None, N=None, K=None, bias=None, R=None, C_out=None, WS=None, ws_w=0.0,
         ws_init=False, a_rowoff=None, c_rowoff=None, lda=None, kc=0, ldk=0, ldw=None, ldc=None,
         ldws=0, act=0, alpha=1.0, post_relu=False, nz=1, zdiv=1, zs=None, precision=0,
         W3=None, a_planes=None, ln_stats=None, ln_colsum=None, W2h=None, col_scale=None,
         a_amax=None, c_amax=None, amax_unit=None, want_row_stats=False, stat_eps=1e-5, mx=False, Wmx=None,
         col_scale_mx=None, kv_col0=None, A2=None, a2_rowoff=None, a2_z0=0, k1=0, k2=0, a2_amax=None,
         stat_bufs=None, kv_bufs=None, amax_guard=0):
    """C = epilogue(A @ W^T); see dzn_gemm_desc.  zs: further descriptor fields by name — the z strides (a_z0, a_z1, w_z0, w_z1,
    c_z0, c_z1, b_z0, b_z1) and the device-chosen subset of the batch, zs=dict(z_list=<int32 tensor>.data_ptr(),
    z_count=<int32 tensor [1]>.data_ptr()): grid row y runs z0 = z_list[y / zdiv] when y / zdiv < z_count[0] and exits otherwise.
    stat_bufs=(partial f32 [M, P, 2], final f32 [M, 2]): caller-owned scratch / result of want_row_stats (else allocated here,
    P = 32); kv_bufs=(planes, inv): caller-owned outputs of kv_col0, planes int16 [2, rows >= M, N - kv_col0].  amax_count (what a
    checked build holds the unit index of a_amax / c_amax against) = the shortest tracker array given, minus amax_guard trailing
    guard entries.  A2 / a2_rowoff / a2_z0 / k1 / k2 / a2_amax: the second A segment (K columns
    k1 .. k1 + k2 read A2[z * a2_z0 + a2_rowoff[m] + k - k1]; a2_amax = its per-unit |max|, computed here when omitted).  kv_col0 (r6): columns >= kv_col0 leave as fp16 two-term planes with per-(row,
    64-column slot) scales instead of fp32 (dzn_gemm_desc.kv_planes) -> returns (C, planes int16 [2, M, N - kv_col0], inv f32
    [M, (N - kv_col0) / 64]).  A: [M, K] (or raw buffer with lda / rowoff),
    W: [N, K] fp32."""
    lib = _lib.load()
    if A.dtype == torch.bfloat16:
        raise ValueError("bf16 A: activations are fp32 (the bf16 engine mode and its contraction are gone)")
    assert A.is_cuda and A.dtype == torch.float32
    if N is None:
        N = W.shape[0]
    if K is None:
        K = W.shape[1]
    if M is None:
        M = A.shape[0]
    if lda is None:
        lda = A.stride(0) if A.dim() == 2 else K
    if ldw is None:
        ldw = W.stride(0)
    if C_out is None:
        C_out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    if ldc is None:
        ldc = C_out.stride(0) if C_out.dim() == 2 else N
    if precision in (_lib.DZN_PREC_F32_SPLIT, _lib.DZN_PREC_F32_H2, _lib.DZN_PREC_F16) and W3 is None and K % 32 == 0 and ldw == K and W.is_contiguous():
        W3 = split_weights(W.reshape(-1, K))   # convenience for tests: engines split once at load
    d = DznGemmDesc()
    d.A, d.W, d.C = _p(A), _p(W), _p(C_out)
    d.bias, d.R, d.WS = _p(bias), _p(R), _p(WS)
    d.a_rowoff, d.c_rowoff = _p(a_rowoff), _p(c_rowoff)
    d.M, d.N, d.K = M, N, K
    d.lda, d.kc, d.ldk, d.ldw, d.ldc, d.ldws = lda, kc, ldk, ldw, ldc, ldws
    d.act, d.alpha, d.post_relu = act, alpha, int(post_relu)
    d.ws_w, d.ws_init = ws_w, int(ws_init)
    d.nz, d.zdiv = nz, zdiv
    if zs:
        for k, v in zs.items():
            setattr(d, k, v)
    d.precision = precision
    d.W3 = _p(W3)
    if a_planes is not None:      # A pre-split by split_rows(): [3, M, K] int16 planes
        d.A = _p(a_planes)
        d.a_split3, d.a_plane = 1, a_planes.stride(0)
    d.ln_stats, d.ln_colsum = _p(ln_stats), _p(ln_colsum)
    if precision in (_lib.DZN_PREC_F32_H2, _lib.DZN_PREC_F16) and W2h is None and K % 32 == 0 and ldw == K and W.is_contiguous():
        W2h, col_scale = split_weights_h2(W.reshape(-1, K))
        if a_amax is None:      # one |max| for the whole tensor, replicated for every z scale unit
            a_amax = amax(A).repeat(max(1, nz // max(zdiv, 1)))
    if mx and Wmx is None:          # DZN_PREC_F16 with fp8 cross terms (csrc/gemm_mx.hip)
        assert precision == _lib.DZN_PREC_F16 and K % 32 == 0 and ldw == K and W.is_contiguous()
        Wmx, col_scale_mx = split_weights_mx(W.reshape(-1, K))
    d.W2h, d.col_scale, d.a_amax, d.c_amax = _p(W2h), _p(col_scale), _p(a_amax), _p(c_amax)
    d.Wmx, d.col_scale_mx = _p(Wmx), _p(col_scale_mx)
    if A2 is not None:
        assert A2.is_cuda and A2.dtype == torch.float32
        if a2_amax is None and a_amax is not None:
            a2_amax = amax(A2.contiguous().reshape(-1)).repeat(max(1, nz // max(zdiv, 1)))
        d.A2, d.a2_rowoff, d.a2_amax = _p(A2), _p(a2_rowoff), _p(a2_amax)
        d.a2_z0, d.k1, d.k2 = a2_z0, k1, k2
    # one scale unit for the whole tensor unless told otherwise (engines use one unit per window)
    d.amax_unit = int(amax_unit) if amax_unit is not None else (max(M, 1) if nz == 1 else 0)
    trackers = [t for t in (a_amax, c_amax, a2_amax if A2 is not None else None) if t is not None]
    if trackers:
        d.amax_count = max(min(t.numel() for t in trackers) - int(amax_guard), 0)
    stats = None
    if want_row_stats:      # LayerNorm statistics of the output rows, left by the epilogue + finalize kernel
        # the epilogue leaves P = column tiles x wavefront columns partials per row; the narrowest wavefront tile of any
        # family is 32 columns, as 64-wide tiles of two wavefront columns or 32-wide tiles of one
        p_max = 2 * ((N + 63) // 64)
        if stat_bufs is not None:
            part, stats = stat_bufs
            assert part.dtype == torch.float32 and stats.dtype == torch.float32
            if part.numel() < M * p_max * 2 or stats.numel() < M * 2:
                raise ValueError(f"want_row_stats: stat_bufs too small for M = {M}, up to {p_max} partials per row")
        else:
            if p_max > 32:
                raise ValueError(f"want_row_stats: N = {N} may leave {p_max} > 32 partials per row; pass stat_bufs")
            part = torch.empty((M, 32, 2), device=A.device, dtype=torch.float32)
            stats = torch.empty((M, 2), device=A.device, dtype=torch.float32)
        d.stat_partial, d.stat_final, d.stat_C, d.stat_eps = _p(part), _p(stats), N, stat_eps
    kvp = kvs = None
    if kv_col0 is not None:
        if kv_bufs is not None:
            kvp, kvs = kv_bufs
            assert kvp.dtype == torch.int16 and kvp.dim() == 3 and kvp.shape[1] >= M and kvp.shape[2] == N - kv_col0
        else:
            kvp = torch.zeros((2, M, N - kv_col0), device=A.device, dtype=torch.int16)
            kvs = torch.zeros((M, (N - kv_col0) // 64), device=A.device, dtype=torch.float32)
        d.kv_planes, d.kv_plane_stride, d.kv_scale, d.kv_ld, d.kv_col0 = _p(kvp), kvp.stride(0), _p(kvs), N - kv_col0, kv_col0
    check(lib.dzn_op_gemm(C.byref(d), _stream()), what="dzn_op_gemm")
    if kv_col0 is not None:
        return C_out, kvp, kvs
    return (C_out, stats) if want_row_stats else C_out


def _window_amax(qkv, B, L, ncols):
    """per-window |max| of the logical [B * L, ncols] part of qkv (which may be a strided view)"""
    return qkv[:B * L, :ncols].reshape(B, -1).abs().amax(dim=1).float().contiguous()


def attention_planes(qkv, B, L, h, gate=None, table=None, head_idx=None, Htot=0, scale=0.125, *, out=None, ldqkv=None, ldo=None,
                     amax=None, planes=None, kvs=None):
    """(r6) csrc/attention_planes.hip through its test entry point: the K / V slots of `qkv` are packed into fp16 two-term planes
    with per-(row, head) power-of-two scales (as the q/k/v contraction's epilogue does) and the planes kernel runs on them.
    out / amax / planes / kvs: caller-owned buffers (out f32 with row stride ldo >= h * 64, amax f32 [B], planes int16 viewed as
    [2, B * L + 64, 2 * h * 64] and kvs f32 [B * L + 64, 2 * h], both zero-filled by the caller); ldqkv / ldo: the row strides, by
    default those of the tensors."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.dtype == torch.float32 and qkv.shape == (B * L, 3 * h * 64)
    ldqkv = qkv.stride(0) if ldqkv is None else int(ldqkv)
    if out is None:
        assert ldo is None
        out = torch.empty((B * L, h * 64), device=qkv.device, dtype=torch.float32)
    ldo = out.stride(0) if ldo is None else int(ldo)
    am = _window_amax(qkv, B, L, 3 * h * 64) if amax is None else amax
    if planes is None:
        planes = torch.zeros((2, B * L + 64, 2 * h * 64), device=qkv.device, dtype=torch.int16)
    if kvs is None:
        kvs = torch.zeros((B * L + 64, 2 * h), device=qkv.device, dtype=torch.float32)
    check(lib.dzn_op_attention_planes(_p(qkv), _p(out), _p(gate), _p(table), _p(head_idx), B, L, h, Htot, ldqkv,
                                      ldo, scale, _p(am), _p(planes), _p(kvs), _stream()), what="dzn_op_attention_planes")
    return out


def split_weights(W):
    """Exact 3-way bf16 split of fp32 weights [rows, K] (K % 32 == 0) for precision=DZN_PREC_F32_SPLIT:
    returns the packed planes as an int16 tensor [rows, K // 32, 3, 32] (csrc/gemm_split.hip)."""
    lib = _lib.load()
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.shape[1] % 32 == 0
    rows, K = W.shape
    out = torch.empty((rows, K // 32, 3, 32), device=W.device, dtype=torch.int16)
    check(lib.dzn_op_split_weights(_p(W), rows, K, W.stride(0), _p(out), _stream()),
          what="dzn_op_split_weights")
    return out


def split_weights_h2(W):
    """two-term fp16 split for precision=DZN_PREC_F32_H2: (planes int16 [rows, K // 32, 2, 32], col_scale f32 [rows])"""
    lib = _lib.load()
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.shape[1] % 32 == 0
    rows, K = W.shape
    out = torch.empty((rows, K // 32, 2, 32), device=W.device, dtype=torch.int16)
    sc = torch.empty((rows,), device=W.device, dtype=torch.float32)
    check(lib.dzn_op_split_weights_h2(_p(W), rows, K, W.stride(0), _p(out), _p(sc), _stream()),
          what="dzn_op_split_weights_h2")
    return out, sc


def split_weights_mx(W):
    """planes of the reduced-precision contraction (DZN_PREC_F16, csrc/gemm_mx.hip): (uint8 [rows, K // 32, 128], col_scale f32 [rows])"""
    lib = _lib.load()
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.shape[1] % 32 == 0
    rows, K = W.shape
    out = torch.empty((rows, K // 32, 128), device=W.device, dtype=torch.uint8)
    sc = torch.empty((rows,), device=W.device, dtype=torch.float32)
    check(lib.dzn_op_split_weights_mx(_p(W), rows, K, W.stride(0), _p(out), _p(sc), _stream()),
          what="dzn_op_split_weights_mx")
    return out, sc


def amax(x, out=None):
    """device scalar max(out, max |x|) — the tracker a producer without a fused one would keep"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    if out is None:
        out = torch.zeros((1,), device=x.device, dtype=torch.float32)
    check(lib.dzn_op_amax(_p(x), x.numel(), _p(out), _stream()), what="dzn_op_amax")
    return out


def split_rows(x):
    """fp32 [rows, D] -> int16 [3, rows, D]: the three bf16 planes of the exact split, fragment order."""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] % 32 == 0
    rows, D = x.shape
    out = torch.empty((3, rows, D), device=x.device, dtype=torch.int16)
    check(lib.dzn_op_split_rows(_p(x), _p(out), out.stride(0), rows, D, _stream()), what="dzn_op_split_rows")
    return out


def conv3x3_c32(img, W3, bias, R=None, relu=False, post_relu=False, out=None, h2_weights=None):
    """3x3 stride-1 conv 32 -> 32 on zero-bordered NHWC fp32 images [B, H+2, W+2, 32] (csrc/conv_split.hip);
    W3 = split_weights(W[32, 288]) with k = (dh*3 + dw)*32 + ci.  Returns a new zero-bordered image."""
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[-1] == 32
    B, Hp, Wp, _ = img.shape
    if out is None:
        out = torch.zeros_like(img)
    if h2_weights is not None:      # fp16 two-term variant: (W2h, col_scale) + per-image |max| of the input
        W2h, cs = h2_weights
        am = img.reshape(B, -1).abs().amax(dim=1).float().contiguous()
        check(lib.dzn_op_conv3x3_c32_h2(_p(img), _p(W3), _p(W2h), _p(cs), _p(am), _p(bias), _p(R), _p(out), B, Hp - 2,
                                        Wp - 2, int(relu), int(post_relu), _stream()), what="dzn_op_conv3x3_c32_h2")
        return out
    check(lib.dzn_op_conv3x3_c32(_p(img), _p(W3), _p(bias), _p(R), _p(out), B, Hp - 2, Wp - 2, int(relu),
                                 int(post_relu), _stream()), what="dzn_op_conv3x3_c32")
    return out


def resblock32_fused(img, h2_w1, b1, h2_w2, b2, l1max1: float, bmax1: float, out=None):
    """one 32-channel BasicBlock, out = relu(conv2(relu(conv1(img) + b1)) + b2 + img), in ONE kernel
    (csrc/resblock_fused.hip): zero-bordered NHWC fp32 images [B, H+2, W+2, 32]; h2_w = split_weights_h2(W[32, 288])
    = (planes, inverse row scales); l1max1 / bmax1 bound the intermediate: max_oc sum_k |W1[oc][k]|, max_oc |b1[oc]|."""
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[-1] == 32
    B, Hp, Wp, _ = img.shape
    if out is None:
        out = torch.zeros_like(img)
    am = img.reshape(B, -1).abs().amax(dim=1).float().contiguous()
    (W1, cs1), (W2, cs2) = h2_w1, h2_w2
    check(lib.dzn_op_resblock32_fused(_p(img), _p(out), _p(W1), _p(cs1), _p(b1), _p(W2), _p(cs2), _p(b2), _p(am),
                                      float(l1max1), float(bmax1), B, Hp - 2, Wp - 2, _stream()),
          what="dzn_op_resblock32_fused")
    return out


def resblock_ws(img, h2_w1, b1, h2_w2, b2, l1max1: float, bmax1: float, out=None):
    """the same block with producer / consumer wavefronts (csrc/resblock_ws.hip), C = img.shape[-1] in (32, 64);
    h2_w = split_weights_h2(W[C, 9 C]) with k = (dh*3 + dw) * C + ci"""
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[-1] in (32, 64)
    B, Hp, Wp, Cn = img.shape
    if out is None:
        out = torch.zeros_like(img)
    am = img.reshape(B, -1).abs().amax(dim=1).float().contiguous()
    (W1, cs1), (W2, cs2) = h2_w1, h2_w2
    check(lib.dzn_op_resblock_ws(_p(img), _p(out), _p(W1), _p(cs1), _p(b1), _p(W2), _p(cs2), _p(b2), _p(am), float(l1max1),
                                 float(bmax1), B, Hp - 2, Wp - 2, Cn, _stream()), what="dzn_op_resblock_ws")
    return out


def _image_ex_args(img, out, amax_in, amax_out, z_count, z_list, channels):
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 4 and img.shape[-1] in channels
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == img.shape
    B = img.shape[0]
    for t, dt in ((amax_in, torch.float32), (amax_out, torch.float32), (z_count, torch.int32), (z_list, torch.int32)):
        assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous())
    assert amax_in is None or amax_in.numel() >= B
    assert amax_out is None or amax_out.numel() >= B
    assert z_count is None or z_count.numel() >= 1
    assert z_list is None or z_list.numel() <= B
    return B, img.shape[1] - 2, img.shape[2] - 2


def conv3x3_c32_ex(img, bias, out, *, W3=None, h2_weights=None, amax_in=None, R=None, relu=False, post_relu=False, amax_out=None,
                   z_count=None, z_list=None):
    """csrc/conv_split.hip in the launch form of the engine (dzn_op_conv3x3_c32_ex): `out` and every tracker are the caller's,
    nothing is filled or allocated.  h2_weights = (W2h, col_scale) with amax_in f32 [B] -> two-term form (W3 may be None), else
    the three-term form on W3.  amax_out f32 [B]: per-image |max| tracker of `out`; z_count int32 [1] / z_list int32 [<= B]: the
    images the launch works on."""
    lib = _lib.load()
    B, H, W = _image_ex_args(img, out, amax_in, amax_out, z_count, z_list, (32,))
    W2h, cs = h2_weights if h2_weights is not None else (None, None)
    check(lib.dzn_op_conv3x3_c32_ex(_p(img), _p(W3), _p(W2h), _p(cs), _p(amax_in), _p(bias), _p(R), _p(out), B, H, W, int(relu),
                                    int(post_relu), _p(amax_out), _p(z_count), _p(z_list), _stream()), what="dzn_op_conv3x3_c32_ex")
    return out


def resblock32_fused_ex(img, h2_w1, b1, h2_w2, b2, l1max1: float, bmax1: float, out, *, amax_in, np=2, amax_out=None, z_count=None,
                        z_list=None):
    """csrc/resblock_fused.hip in the launch form of the engine (dzn_op_resblock32_fused_ex): caller-owned `out`, amax_in f32 [B],
    optional tracker and image list, np = terms per operand (2 or 1)."""
    lib = _lib.load()
    B, H, W = _image_ex_args(img, out, amax_in, amax_out, z_count, z_list, (32,))
    (W1, cs1), (W2, cs2) = h2_w1, h2_w2
    check(lib.dzn_op_resblock32_fused_ex(_p(img), _p(out), _p(W1), _p(cs1), _p(b1), _p(W2), _p(cs2), _p(b2), _p(amax_in), _p(amax_out),
                                         float(l1max1), float(bmax1), B, H, W, int(np), _p(z_count), _p(z_list), _stream()),
          what="dzn_op_resblock32_fused_ex")
    return out


def resblock_ws_ex(img, h2_w1, b1, h2_w2, b2, l1max1: float, bmax1: float, out, *, amax_in, np=2, amax_out=None, z_count=None,
                   z_list=None, C_planes=None):
    """csrc/resblock_ws.hip in the launch form of the engine (dzn_op_resblock_ws_ex); C_planes: the channel count handed to the
    library, by default the images' (a test of the refusal passes another)."""
    lib = _lib.load()
    B, H, W = _image_ex_args(img, out, amax_in, amax_out, z_count, z_list, (32, 64))
    (W1, cs1), (W2, cs2) = h2_w1, h2_w2
    Cn = img.shape[-1] if C_planes is None else int(C_planes)
    check(lib.dzn_op_resblock_ws_ex(_p(img), _p(out), _p(W1), _p(cs1), _p(b1), _p(W2), _p(cs2), _p(b2), _p(amax_in), _p(amax_out),
                                    float(l1max1), float(bmax1), B, H, W, Cn, int(np), _p(z_count), _p(z_list), _stream()),
          what="dzn_op_resblock_ws_ex")
    return out


def linkage_centroid(emb, device: int = -1):
    """scipy.cluster.hierarchy.linkage(emb, "centroid", "euclidean") on the device (csrc/linkage.hip):
    emb = host float32 [n, dim] (numpy), returns the dendrogram float64 [n - 1, 4]."""
    import numpy as np
    lib = _lib.load()
    e = np.ascontiguousarray(emb, dtype=np.float32)
    n, dim = e.shape
    Z = np.empty((n - 1, 4), dtype=np.float64)
    check(lib.dzn_linkage_centroid(e.ctypes.data_as(C.c_void_p), n, dim, Z.ctypes.data_as(C.c_void_p), device),
          what="dzn_linkage_centroid")
    return Z


def link_speakers(emb, group, threshold: float, device: int = -1):
    """Complete linkage of cosine distances under a cannot-link constraint, cut at `threshold`, on the device (csrc/linkage.hip,
    dzn_link_speakers): emb = host float32 [n, dim], group = int32 [n] (rows of one group never merge), threshold a cosine
    distance in (0, 2].  Returns (Z_prefix float64 [m, 4], m): exactly the merges of height <= threshold of
        y = pdist(emb.astype(float64), "cosine"); y[same group] = 4.0; linkage(y, "complete")
    in scipy's order.  Bad shapes or arguments raise DznError (the library's DZN_E_INVALID), a matrix that does not fit raises
    MemoryError."""
    import numpy as np
    lib = _lib.load()
    e = np.ascontiguousarray(emb, dtype=np.float32)
    g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
    if e.ndim != 2 or g.shape[0] != e.shape[0]:
        raise ValueError(f"link_speakers: emb is [n, dim] and group [n], not {e.shape} and {g.shape}")
    n, dim = e.shape
    Z = np.empty((max(n - 1, 1), 4), dtype=np.float64)
    m = C.c_int32(0)
    check(lib.dzn_link_speakers(e.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), n, dim, float(threshold),
                                Z.ctypes.data_as(C.c_void_p), C.byref(m), device), what="dzn_link_speakers")
    return Z[:m.value].copy(), int(m.value)


def link_speakers_last():
    """diagnostics of the last link_speakers call of the process: {launches, merges, rescans, pdist_ms} (the step launches
    queued, surplus ones included; the distance kernel alone by HIP events)"""
    lib = _lib.load()
    launches, merges, rescans, ms = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_float(0.0)
    check(lib.dzn_link_speakers_last(C.byref(launches), C.byref(merges), C.byref(rescans), C.byref(ms)),
          what="dzn_link_speakers_last")
    return {"launches": launches.value, "merges": merges.value, "rescans": rescans.value, "pdist_ms": ms.value}


def cdist_cosine(emb, centroids, device: int = -1):
    """scipy.spatial.distance.cdist(emb, centroids, "cosine") on the device in scipy's float64 operation order
    (csrc/linkage.hip): emb = host float32 [n, dim], centroids [k, dim] -> float64 [n, k]."""
    import numpy as np
    lib = _lib.load()
    e = np.ascontiguousarray(emb, dtype=np.float32)
    c = np.ascontiguousarray(centroids, dtype=np.float64)
    n, dim = e.shape
    k = c.shape[0]
    assert c.shape[1] == dim
    out = np.empty((n, k), dtype=np.float64)
    check(lib.dzn_cdist_cosine(e.ctypes.data_as(C.c_void_p), n, dim, c.ctypes.data_as(C.c_void_p), k,
                               out.ctypes.data_as(C.c_void_p), device), what="dzn_cdist_cosine")
    return out


class VbxState:
    """the E-sized arrays of the VBx mixture resident on the device (csrc/vbx.hip): X f64 [E, D], Phi f64 [D],
    gamma0 f64 [E, K]; see diarizen_amd/clustering.py:vb_gmm for the loop that drives it."""

    def __init__(self, X, Phi, gamma0, device: int = -1):
        import numpy as np
        self.np, self.lib = np, _lib.load()
        X = np.ascontiguousarray(X, dtype=np.float64)
        Phi = np.ascontiguousarray(Phi, dtype=np.float64)
        g0 = np.ascontiguousarray(gamma0, dtype=np.float64)
        self.E, self.D = X.shape
        self.K = g0.shape[1]
        assert Phi.shape == (self.D,) and g0.shape[0] == self.E
        self.state = C.c_void_p()
        check(self.lib.dzn_vbx_create(X.ctypes.data_as(C.c_void_p), Phi.ctypes.data_as(C.c_void_p),
                                      g0.ctypes.data_as(C.c_void_p), self.E, self.D, self.K, device,
                                      C.byref(self.state)), what="dzn_vbx_create")

    def stats(self):
        out = self.np.empty((self.K, self.D + 1), dtype=self.np.float64)
        check(self.lib.dzn_vbx_stats(self.state, out.ctypes.data_as(C.c_void_p)), what="dzn_vbx_stats")
        return out

    def estep(self, alpha, ck, lpi, Fa: float) -> float:
        np = self.np
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        ck = np.ascontiguousarray(ck, dtype=np.float64)
        lpi = np.ascontiguousarray(lpi, dtype=np.float64)
        assert alpha.shape == (self.K, self.D) and ck.shape == (self.K,) and lpi.shape == (self.K,)
        total = C.c_double(0.0)
        check(self.lib.dzn_vbx_estep(self.state, alpha.ctypes.data_as(C.c_void_p), ck.ctypes.data_as(C.c_void_p),
                                     lpi.ctypes.data_as(C.c_void_p), float(Fa), C.byref(total)), what="dzn_vbx_estep")
        return total.value

    def gamma(self):
        out = self.np.empty((self.E, self.K), dtype=self.np.float64)
        check(self.lib.dzn_vbx_gamma(self.state, out.ctypes.data_as(C.c_void_p)), what="dzn_vbx_gamma")
        return out

    def close(self):
        if self.state:
            self.lib.dzn_vbx_destroy(self.state)
            self.state = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # pragma: no cover
            pass


class GalleryState:
    """a device-resident gallery of L2-normalised fp32 rows and the cosine search over it (csrc/gallery.hip): host arrays in,
    host arrays out; see diarizen_amd/identification.py:SpeakerGallery for the bookkeeping that drives it."""

    def __init__(self, dim: int, capacity: int, device: int = -1):
        import numpy as np
        self.np, self.lib = np, _lib.load()
        self.dim, self.capacity = int(dim), int(capacity)
        self.state = C.c_void_p()
        check(self.lib.dzn_gallery_create(device, self.dim, self.capacity, C.byref(self.state)), what="dzn_gallery_create")
        g = [C.c_int32(0) for _ in range(4)]
        check(self.lib.dzn_gallery_geometry(self.state, *[C.byref(v) for v in g]), what="dzn_gallery_geometry")
        self.tile_rows, self.sweep_rows, self.query_group, self.max_top_n = (v.value for v in g)

    @property
    def rows(self) -> int:
        """highest slot ever put + 1: the width of the dense output"""
        n = C.c_int64(0)
        check(self.lib.dzn_gallery_rows(self.state, C.byref(n)), what="dzn_gallery_rows")
        return n.value

    def put(self, slot: int, vecs) -> None:
        v = self.np.ascontiguousarray(vecs, dtype=self.np.float32).reshape(-1, self.dim)
        check(self.lib.dzn_gallery_put(self.state, int(slot), v.ctypes.data_as(C.c_void_p), v.shape[0]), what="dzn_gallery_put")

    def drop(self, slot: int, count: int = 1) -> None:
        check(self.lib.dzn_gallery_drop(self.state, int(slot), int(count)), what="dzn_gallery_drop")

    def search(self, queries, top_n: int, dense: bool = False):
        """queries f32 [Q, dim] -> (scores f32 [Q, top_n], slots i64 [Q, top_n]) (+ every score f32 [Q, rows] with dense=True)"""
        np = self.np
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        Q = q.shape[0]
        scores = np.empty((Q, int(top_n)), dtype=np.float32)
        slots = np.empty((Q, int(top_n)), dtype=np.int64)
        d = np.empty((Q, self.rows), dtype=np.float32) if dense else None
        check(self.lib.dzn_gallery_search(self.state, q.ctypes.data_as(C.c_void_p), Q, int(top_n),
                                          scores.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p),
                                          d.ctypes.data_as(C.c_void_p) if dense else None), what="dzn_gallery_search")
        return (scores, slots, d) if dense else (scores, slots)

    def last_launch_ms(self):
        """(HIP-event time of the last search's launches, the share of its last merge), in ms"""
        ms, merge = C.c_float(0.0), C.c_float(0.0)
        check(self.lib.dzn_gallery_last_launch_ms(self.state, C.byref(ms), C.byref(merge)), what="dzn_gallery_last_launch_ms")
        return ms.value, merge.value

    def close(self):
        if self.state:
            self.lib.dzn_gallery_destroy(self.state)
            self.state = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # pragma: no cover
            pass


class Registry:
    """a device-resident, growing set of speaker identities and the match of a recording's voiceprints against it
    (csrc/registry.hip): host arrays in, host arrays out; see diarizen_amd/registry.py:SpeakerRegistry for the rule that
    drives it."""

    def __init__(self, dim: int, capacity: int, device: int = -1):
        import numpy as np
        self.np, self.lib = np, _lib.load()
        self.dim, self.capacity = int(dim), int(capacity)
        self.state = C.c_void_p()
        check(self.lib.dzn_registry_create(device, self.dim, self.capacity, C.byref(self.state)), what="dzn_registry_create")

    def _counts(self):
        n, i = C.c_int64(0), C.c_int64(0)
        check(self.lib.dzn_registry_rows(self.state, C.byref(n), C.byref(i)), what="dzn_registry_rows")
        return n.value, i.value

    @property
    def rows(self) -> int:
        return self._counts()[0]

    @property
    def identities(self) -> int:
        """the highest identity number appended + 1: the width of the dense table"""
        return self._counts()[1]

    def append(self, vecs, identity) -> None:
        np = self.np
        v = np.ascontiguousarray(vecs, dtype=np.float32).reshape(-1, self.dim)
        i = np.ascontiguousarray(identity, dtype=np.int32).reshape(-1)
        if len(i) != len(v):
            raise ValueError(f"Registry.append: one identity per row ({len(v)} rows, {len(i)} identities)")
        check(self.lib.dzn_registry_append(self.state, v.ctypes.data_as(C.c_void_p), len(v), i.ctypes.data_as(C.c_void_p)),
              what="dzn_registry_append")

    def match(self, queries, threshold: float, dense: bool = False, max_out: int = 0):
        """queries f32 [Q, dim] -> (k i32 [m], identity i32 [m], d f64 [m]): the entries <= threshold of the table
        D[k, i] = max over the rows of identity i of the cosine distance to query k, sorted by (k, i)  (+ the table itself,
        f64 [Q, identities], with dense=True)"""
        np = self.np
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        Q = q.shape[0]
        width = self.identities
        table = np.empty((Q, width), dtype=np.float64) if dense else None
        # room for every entry of the table up to 2^16 triples (1 MB): a second sweep only beyond that, or under a small max_out
        room = int(max_out) if max_out > 0 else max(1, min(Q * width, 1 << 16))
        while True:
            k, i, d = np.empty(room, dtype=np.int32), np.empty(room, dtype=np.int32), np.empty(room, dtype=np.float64)
            m = C.c_int32(0)
            check(self.lib.dzn_registry_match(self.state, q.ctypes.data_as(C.c_void_p), Q, float(threshold), room,
                                              k.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p),
                                              d.ctypes.data_as(C.c_void_p), C.byref(m),
                                              table.ctypes.data_as(C.c_void_p) if dense else None), what="dzn_registry_match")
            if m.value <= room:
                break
            room = m.value              # more entries than room: once more with room for all
        out = (k[:m.value].copy(), i[:m.value].copy(), d[:m.value].copy())
        return out + (table,) if dense else out

    def last_launch_ms(self) -> float:
        """HIP-event time of the last match's launches, in ms"""
        ms = C.c_float(0.0)
        check(self.lib.dzn_registry_last_launch_ms(self.state, C.byref(ms)), what="dzn_registry_last_launch_ms")
        return ms.value

    def close(self):
        if self.state:
            self.lib.dzn_registry_destroy(self.state)
            self.state = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # pragma: no cover
            pass


def layernorm(x, gamma, beta, C_true=None, eps=1e-5, gelu=False, out=None):
    lib = _lib.load()
    rows, ld = x.shape[0], x.stride(0)
    Cpad = x.shape[1]
    if C_true is None:
        C_true = Cpad
    if out is None:
        out = torch.empty_like(x)
    check(lib.dzn_op_layernorm(_p(x), ld, _p(out), out.stride(0), _p(gamma), _p(beta), rows,
                               C_true, Cpad, eps, int(gelu), _stream()), what="dzn_op_layernorm")
    return out


def row_stats(x, C_true=None, eps=1e-5):
    """(mean, rstd) per row of x[:, :C_true] -> f32 [rows, 2] (the LayerNorm folded into a contraction)"""
    lib = _lib.load()
    rows = x.shape[0]
    out = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
    check(lib.dzn_op_row_stats(_p(x), x.stride(0), rows, C_true or x.shape[1], eps, _p(out), _stream()),
          what="dzn_op_row_stats")
    return out


def gate_stats(x, gamma, beta, Wg, bg, cst, eps=1e-5, out=None):
    """one pass over raw rows x [rows, Htot*64]: (gate [rows, Htot] on LayerNorm(x), stats [rows, 2]); out = caller-owned
    (gate, stats), both contiguous"""
    lib = _lib.load()
    rows, Htot = x.shape[0], cst.numel()
    if out is None:
        out = (torch.empty((rows, Htot), device=x.device, dtype=torch.float32),
               torch.empty((rows, 2), device=x.device, dtype=torch.float32))
    gate_, stats = out
    check(lib.dzn_op_gate_stats(_p(x), x.stride(0), _p(gamma), _p(beta), _p(Wg), _p(bg), _p(cst), _p(gate_), _p(stats),
                                rows, Htot, eps, _stream()), what="dzn_op_gate_stats")
    return gate_, stats


def stats_finalize(partial, C, eps=1e-5, out=None):
    """(mean, rstd) f32 [rows, 2] of rows of C elements from the partials f32 [rows, P, 2] (sum, sum of squares) a contraction
    epilogue left (dzn_gemm_desc.stat_partial): what the contraction launcher runs when stat_final is set"""
    lib = _lib.load()
    rows, P = partial.shape[0], partial.shape[1]
    assert partial.is_contiguous() and partial.dtype == torch.float32 and partial.shape[2] == 2
    if out is None:
        out = torch.empty((rows, 2), device=partial.device, dtype=torch.float32)
    check(lib.dzn_op_stats_finalize(_p(partial), rows, P, C, eps, _p(out), _stream()), what="dzn_op_stats_finalize")
    return out


def gate_heads(x, gamma, beta, Wg, bg, cst, head_idx, partial, eps=1e-5, out=None, h=None, P=None):
    """gate_stats for rows whose LayerNorm partial sums are given (partial f32 [rows, P, 2], P <= 32): stats [rows, 2] from the
    partials, and gate[:, H] for the heads H in head_idx (int32, device) from their 64 channels of x alone; the other columns
    of gate keep what they held.  out = caller-owned (gate [rows, Htot], stats), both contiguous; h / P override the counts
    taken from head_idx / partial (tests of the argument checks)."""
    lib = _lib.load()
    rows, Htot = x.shape[0], cst.numel()
    assert head_idx.dtype == torch.int32 and partial.dtype == torch.float32 and partial.is_contiguous()
    if out is None:
        out = (torch.empty((rows, Htot), device=x.device, dtype=torch.float32),
               torch.empty((rows, 2), device=x.device, dtype=torch.float32))
    gate_, stats = out
    check(lib.dzn_op_gate_heads(_p(x), x.stride(0), _p(gamma), _p(beta), _p(Wg), _p(bg), _p(cst), _p(head_idx),
                                head_idx.numel() if h is None else h, _p(partial), partial.shape[1] if P is None else P,
                                Htot * 64, eps, _p(gate_), _p(stats), rows, Htot, _stream()), what="dzn_op_gate_heads")
    return gate_, stats


def gate(y, Wg, bg, cst, out=None):
    lib = _lib.load()
    rows = y.shape[0]
    Htot = cst.numel()
    if out is None:
        out = torch.empty((rows, Htot), device=y.device, dtype=torch.float32)
    check(lib.dzn_op_gate(_p(y), y.stride(0), _p(Wg), _p(bg), _p(cst), _p(out), rows, Htot,
                          _stream()), what="dzn_op_gate")
    return out


def attention(qkv, B, L, h, *, gate=None, table=None, head_idx=None, Htot=0, scale=0.125,
              precision=0, out=None, ldqkv=None, ldo=None, amax=None):
    """out / amax: caller-owned buffers (out f32 with row stride ldo >= h * 64; amax f32 [B], the per-window |max| the fp16
    two-term variant scales by); ldqkv / ldo: the row strides, by default those of the tensors (qkv may be a strided view)"""
    lib = _lib.load()
    ldqkv = qkv.stride(0) if ldqkv is None else int(ldqkv)
    if out is None:
        assert ldo is None
        out = torch.empty((B * L, h * 64), device=qkv.device, dtype=torch.float32)
    ldo = out.stride(0) if ldo is None else int(ldo)
    if precision == _lib.DZN_PREC_F32_H2:      # fp16 two-term variant: per-window |max| of qkv
        am = _window_amax(qkv, B, L, 3 * h * 64) if amax is None else amax
        check(lib.dzn_op_attention_h2(_p(qkv), _p(out), _p(gate), _p(table), _p(head_idx), B, L, h, Htot,
                                      ldqkv, ldo, scale, _p(am), _stream()), what="dzn_op_attention_h2")
        return out
    check(lib.dzn_op_attention(_p(qkv), _p(out), _p(gate), _p(table), _p(head_idx), B, L, h,
                               Htot, ldqkv, ldo, scale, precision, _stream()),
          what="dzn_op_attention")
    return out


# ---- the small kernels (conformer.hip, frontend.hip, norm.hip, embed.hip): thin wrappers for tests/test_small_kernels_gpu.py.
# Outputs and row strides are the caller's (a tensor argument may be a view into a larger, pattern-filled buffer); nothing is
# allocated or reshaped here unless an output is omitted, and a launcher's refusal surfaces as DznError.

def layernorm_t(x, gamma, beta, *, rows, C, Cpad, ldx, out, ldy, post=None, eps=1e-5, gelu=False, amax=None, amax_unit=0):
    """launch_layernorm_t in full: out may be x (in place); post f32 [C]; amax f32 [units] with unit = row // amax_unit
    (amax_unit == 0: one unit)"""
    lib = _lib.load()
    check(lib.dzn_op_layernorm_t(_p(x), int(ldx), _p(out), int(ldy), _p(gamma), _p(beta), _p(post), int(rows), int(C), int(Cpad),
                                 eps, int(gelu), _p(amax), int(amax_unit), _stream()), what="dzn_op_layernorm_t")
    return out


def wave_stats(w, B, N, eps=1e-5, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty((B, 2), device=w.device, dtype=torch.float32)
    check(lib.dzn_op_wave_stats(_p(w), int(B), int(N), eps, _p(out), _stream()), what="dzn_op_wave_stats")
    return out


def glu_dwconv(u, w, bias, out, *, B, L, A, ks, ldu, ldo):
    lib = _lib.load()
    check(lib.dzn_op_glu_dwconv(_p(u), int(ldu), _p(w), _p(bias), _p(out), int(ldo), int(B), int(L), int(A), int(ks), _stream()),
          what="dzn_op_glu_dwconv")
    return out


def classify(z, W, bias, mapping, *, rows, A, NC, S, ldz, logp=None, multilabel=None, soft=None):
    """mapping u8 [NC, S]; logp f32 [rows, NC], multilabel u8 [rows, S], soft f32 [rows, S]: each optional"""
    lib = _lib.load()
    check(lib.dzn_op_classify(_p(z), int(ldz), _p(W), _p(bias), _p(mapping), int(rows), int(A), int(NC), int(S), _p(logp),
                              _p(multilabel), _p(soft), _stream()), what="dzn_op_classify")
    return logp, multilabel, soft


def gn_stats_floats(B, T, C, Cp) -> int:
    return int(_lib.load().dzn_op_gn_stats_floats(int(B), int(T), int(C), int(Cp)))


def groupnorm_gelu(x, y, gamma, beta, stats, *, B, T, C, Cp, ld, eps=1e-5, amax=None):
    """stats: f32 scratch of gn_stats_floats(B, T, C, Cp) floats; y may be x"""
    lib = _lib.load()
    check(lib.dzn_op_groupnorm_gelu(_p(x), _p(y), int(B), int(T), int(C), int(Cp), int(ld), _p(gamma), _p(beta), eps, _p(stats),
                                    _p(amax), _stream()), what="dzn_op_groupnorm_gelu")
    return y


def conv0_lnq(w, C0, k):
    """HOST: w = numpy float32 [C0, k] -> numpy float32 [110]: (wbar [10], F [10, 10]) of dzn_op_conv0_lnq; no device involved"""
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.full(110, np.nan, np.float32)
    check(_lib.load().dzn_op_conv0_lnq(C.c_void_p(w.ctypes.data), int(C0), int(k), C.c_void_p(out.ctypes.data)), what="dzn_op_conv0_lnq")
    return out


def conv0(wave, w, out, *, B, N, C0, Cp, k, s, T0, layer_norm, stats=None, gamma=None, beta=None, lnq=None, eps=1e-5):
    """out [B, T0, Cp] = conv0 of wave [B, N] (csrc/frontend.hip); layer_norm: LayerNorm over C0 + GELU, statistics from lnq or,
    without it, from the frame's outputs"""
    lib = _lib.load()
    check(lib.dzn_op_conv0(_p(wave), int(B), int(N), _p(stats), _p(w), _p(gamma), _p(beta), int(C0), int(Cp), int(k), int(s), int(T0),
                           int(layer_norm), eps, _p(out), _p(lnq), _stream()), what="dzn_op_conv0")
    return out


def split_weights_h2_frag(W, out=None, col_scale=None):
    """split_weights_h2 in the fragment-major order conv01_fused reads: (planes int16 [K // 32, rows // 16, 2, 16, 32], col_scale)"""
    lib = _lib.load()
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous()
    rows, K = W.shape
    if out is None:
        out = torch.empty((max(K // 32, 1), max(rows // 16, 1), 2, 16, 32), device=W.device, dtype=torch.int16)
    if col_scale is None:
        col_scale = torch.empty((rows,), device=W.device, dtype=torch.float32)
    check(lib.dzn_op_split_weights_h2_frag(_p(W), rows, K, _p(out), _p(col_scale), _stream()), what="dzn_op_split_weights_h2_frag")
    return out, col_scale


def conv01_fused(wave, w0, gamma0, beta0, lnq, W2h, col_scale, out, *, B, N, C0, T0, T1, act_bound, N1p=160, wstats=None, gamma1=None,
                 beta1=None, C1=0, amax1=None, eps=1e-5):
    """out [B, T1, N1p] = conv1(GELU(LN(conv0(wave)))) in one kernel (csrc/frontend_fused.hip); gamma1 / beta1: + LN over C1 + GELU"""
    lib = _lib.load()
    check(lib.dzn_op_conv01_fused(_p(wave), int(B), int(N), _p(wstats), _p(w0), _p(gamma0), _p(beta0), _p(lnq), int(C0), int(T0), int(T1),
                                  _p(W2h), _p(col_scale), int(N1p), float(act_bound), eps, _p(out), _p(gamma1), _p(beta1), int(C1),
                                  _p(amax1), _stream()), what="dzn_op_conv01_fused")
    return out


def pad_rows(x, xpad, *, B, L, Lp, pad, D):
    lib = _lib.load()
    check(lib.dzn_op_pad_rows(_p(x), _p(xpad), int(B), int(L), int(Lp), int(pad), int(D), _stream()), what="dzn_op_pad_rows")
    return xpad


def pad_rows_split2(x, amax, *, B, L, taps, G, cg, cgp=64):
    """x fp32 [B * L, G * cg], amax f32 [B] (>= the windows' |max|) -> (planes int16 [2, B * (L + taps), G * cgp], snapshot f32 [B]):
    the fp16 two-term planes of the zero-padded copy the positional conv reads (dzn_op_pad_rows_split2)"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * L * G * cg
    Lp = L + taps
    planes = torch.empty((2, B * Lp, G * cgp), device=x.device, dtype=torch.int16)
    snap = torch.empty((B,), device=x.device, dtype=torch.float32)
    check(lib.dzn_op_pad_rows_split2(_p(x), _p(planes), planes.stride(0), int(B), int(L), int(Lp), int(taps // 2), int(G * cgp),
                                     _p(amax), _p(snap), int(cg), int(cgp), _stream()), what="dzn_op_pad_rows_split2")
    return planes, snap


def posconv_resident_fits(B, L, taps) -> bool:
    return bool(_lib.load().dzn_op_posconv_resident_fits(int(B), int(L), int(taps)))


def posconv(planes, snap, W, h2_weights, *, B, L, taps, G, cg, bias=None, R=None, out=None, act=0, c_amax=None, resident=True):
    """The positional conv over the planes of pad_rows_split2 (64 plane channels per group): out[b L + t, g cg + n] =
    epilogue(sum_j sum_c planes[b, t + j, g 64 + c] W[g cg + n, j 64 + c]), W fp32 [G * cg, taps * 64] and h2_weights =
    split_weights_h2(W).  resident=True: csrc/posconv_resident.hip (dzn_op_posconv_resident); False: the generic pre-split
    contraction with its row-offset table (dzn_op_gemm) on the same descriptor."""
    lib = _lib.load()
    W2h, wsc = h2_weights
    D, Dp, Lp, K = G * cg, planes.shape[2], L + taps, taps * 64
    assert planes.dtype == torch.int16 and planes.shape == (2, B * Lp, G * 64) and W.shape == (D, K) and W.is_contiguous()
    if out is None:
        out = torch.empty((B * L, D), device=planes.device, dtype=torch.float32)
    rowoff = ((torch.arange(B, device=planes.device, dtype=torch.int64)[:, None] * Lp
               + torch.arange(L, device=planes.device, dtype=torch.int64)[None, :]) * Dp).to(torch.int32).reshape(-1).contiguous()
    d = DznGemmDesc()
    d.A, d.W, d.C, d.bias, d.R = _p(planes), _p(W), _p(out), _p(bias), _p(R)
    d.M, d.N, d.K = B * L, cg, K
    d.lda, d.kc, d.ldk, d.ldw, d.ldc = Dp, 64, Dp, K, D
    d.act, d.alpha = act, 1.0
    d.nz, d.zdiv = G, G
    d.a_z1, d.w_z1, d.c_z1, d.b_z1 = 64, cg * K, cg, cg
    d.a_rowoff = _p(rowoff)
    d.precision = _lib.DZN_PREC_F32_H2
    d.a_split3, d.a_plane = 2, planes.stride(0)
    d.W2h, d.col_scale, d.a_amax, d.c_amax = _p(W2h), _p(wsc), _p(snap), _p(c_amax)
    d.amax_unit = L
    d.amax_count = B
    if resident:
        check(lib.dzn_op_posconv_resident(C.byref(d), int(B), int(L), int(taps), _stream()), what="dzn_op_posconv_resident")
    else:
        check(lib.dzn_op_gemm(C.byref(d), _stream()), what="dzn_op_gemm")
    return out


def ws_accum(x, ws, w, init, n):
    lib = _lib.load()
    check(lib.dzn_op_ws_accum(_p(x), _p(ws), float(w), int(bool(init)), int(n), _stream()), what="dzn_op_ws_accum")
    return ws


def ws_sum(xs, weights, ws, n):
    """xs: list of device tensors, weights: list of floats (the launch takes them by value)"""
    lib = _lib.load()
    k = len(xs)
    ptrs = (C.c_void_p * max(k, 1))(*[x.data_ptr() for x in xs])
    wts = (C.c_float * max(k, 1))(*[float(w) for w in weights])
    check(lib.dzn_op_ws_sum(ptrs, wts, k, _p(ws), int(n), _stream()), what="dzn_op_ws_sum")
    return ws


def col_scale(x, scale, *, rows, C_true, ld):
    lib = _lib.load()
    check(lib.dzn_op_col_scale(_p(x), int(rows), int(C_true), int(ld), _p(scale), _stream()), what="dzn_op_col_scale")
    return x


def frame_prep(wave, window, frames, *, B, stride, T, flen, fshift, Kp, preemph=0.97):
    lib = _lib.load()
    check(lib.dzn_op_frame_prep(_p(wave), int(B), int(stride), int(T), int(flen), int(fshift), int(Kp), _p(window), preemph,
                                _p(frames), _stream()), what="dzn_op_frame_prep")
    return frames


def power(spec, pw, *, rows, nb):
    lib = _lib.load()
    check(lib.dzn_op_power(_p(spec), int(rows), int(nb), _p(pw), _stream()), what="dzn_op_power")
    return pw


def log_cmn(mel, *, B, T, NB, eps):
    lib = _lib.load()
    check(lib.dzn_op_log_cmn(_p(mel), int(B), int(T), int(NB), eps, _stream()), what="dzn_op_log_cmn")
    return mel


def log_cmn_gather(mel, fb, *, q, B, T, NB, eps):
    lib = _lib.load()
    check(lib.dzn_op_log_cmn_gather(_p(mel), int(q), _p(fb), int(B), int(T), int(NB), eps, _stream()), what="dzn_op_log_cmn_gather")
    return fb


def stem_conv(fb, w, bias, img, *, B, T, NB, C_out, amax=None, z_count=None, z_list=None):
    lib = _lib.load()
    check(lib.dzn_op_stem_conv(_p(fb), int(B), int(T), int(NB), int(C_out), _p(w), _p(bias), _p(img), _p(amax), _p(z_count),
                               _p(z_list), _stream()), what="dzn_op_stem_conv")
    return img


def stats_pool(img, masks, stats, *, B, H, W, C_in, S, L, active=None):
    lib = _lib.load()
    check(lib.dzn_op_stats_pool(_p(img), int(B), int(H), int(W), int(C_in), _p(masks), int(S), int(L), _p(stats), _p(active),
                                _stream()), what="dzn_op_stats_pool")
    return stats


def window_active(masks, flag, *, B, per_window):
    lib = _lib.load()
    check(lib.dzn_op_window_active(_p(masks), int(B), int(per_window), _p(flag), _stream()), what="dzn_op_window_active")
    return flag


def compact_active(flag, count, lst, *, B, totals=None):
    """count i32 [1], lst i32 [>= B], totals i64 [2] or None (accumulates)"""
    lib = _lib.load()
    check(lib.dzn_op_compact_active(_p(flag), int(B), _p(count), _p(lst), _p(totals), _stream()), what="dzn_op_compact_active")
    return count, lst


def ingest_many(stage, desc, banks, pool):
    """dzn_ingest_many on the current stream: ONE launch over the descriptor table `desc` (a numpy record array of
    _lib.ingest_desc_dtype(), validated by the library from this host image and uploaded here), sources in `stage` (u8 device
    tensor), banks in `banks` (f32 device tensor or None), outputs into `pool` (f32 device tensor [rows, row_floats])"""
    import numpy as np
    lib = _lib.load()
    desc = np.ascontiguousarray(desc, dtype=_lib.ingest_desc_dtype()).reshape(-1)
    assert pool.dim() == 2 and pool.is_contiguous() and pool.dtype == torch.float32 and stage.dtype == torch.uint8
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(pool.device)
    dev = pool.device.index if pool.device.index is not None else -1
    check(lib.dzn_ingest_many(dev, _p(stage), stage.numel(), C.c_void_p(desc.ctypes.data), _p(d_desc), len(desc), _p(banks),
                              0 if banks is None else banks.numel(), _p(pool), pool.shape[0], pool.shape[1], _stream()),
          what="dzn_ingest_many")
    return pool


def gather_windows(pool, offsets, window, out=None):
    """dzn_gather_windows on the current stream: out f32 [B, window], out[b] = pool.view(-1)[offsets[b] : offsets[b] + window]
    (offsets: a host sequence of float offsets; the library validates them against the pool's size)"""
    import numpy as np
    lib = _lib.load()
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    B = len(off)
    assert pool.is_contiguous() and pool.dtype == torch.float32
    if out is None:
        out = torch.empty((B, int(window)), device=pool.device, dtype=torch.float32)
    d_off = torch.from_numpy(off.copy()).to(pool.device) if B else None
    dev = pool.device.index if pool.device.index is not None else -1
    check(lib.dzn_gather_windows(dev, _p(pool), pool.numel(), C.c_void_p(off.ctypes.data), _p(d_off), B, int(window), _p(out),
                                 _stream()), what="dzn_gather_windows")
    return out
