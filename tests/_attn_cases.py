"""Shared by test_attention_matrix_gpu.py (device) and test_attention_bounds_host.py (CPU): the case table of the attention
family (csrc/attention.hip, attention_split.hip, attention_planes.hip), its inputs, the float64 reference of a launch and the
per-element error bound that goes with it.  torch only; nothing here touches a device.

Forms, by entry point: "f32" dzn_op_attention at precision 0 (fp32 MFMA), "f32s" dzn_op_attention at the split precision (bf16
three-term), "f32h_split" dzn_op_attention_h2 (fp16 two-term, ONE power-of-two scale per window), "planes"
dzn_op_attention_planes (K / V packed per (row, head), Q on the window scale) under its three schedule forms.

The bound is per output element and DERIVED, never tuned.  u = 2^-24.  With s_ik = scale q_i.k_k + g_i T[k - i + L - 1] the
float64 scores, m_i their row maximum, p_ik the float64 probabilities, l_i = sum_k exp(s_ik - m_i) >= 1, N_id = sum_k p_ik
|v_kd| and S1_ik = scale sum_d |q_id| |k_kd|:

  score error D_ik (in natural-log units; the log2-domain kernels carry the factor log2 e through, which cancels):
      accumulation      (64 + 8) u S1      fp32 accumulation over 64 products, as _gemm_cases.py counts it
                        + 2 u S1           q times (scale log2 e): the constant's rounding and the product's
      operands          f32, f32s: nothing (fp32 operands; the bf16 three-term split is exact)
                        f32h_split: 2^-21 S1 + 2^-38 amax_w (sum_d |k_kd| + scale sum_d |q_id|): 22 bits kept per operand and the
                                    floor of the lo term on the fp16 subnormal grid relative to the WINDOW maximum (split.h, as
                                    _gemm_cases.py counts it)
                        planes:     2^-21 S1 + 2^-38 (amax_w sum_d |k_kd| + amax(k_k) scale sum_d |q_id|): Q on the window
                                    scale, K on the scale of its own (row, head)
      bias              3 u |g T| + u |s|   g log2 e (constant, product), then one fma whose result is rounded once
  probability error: the un-normalised exp(s_ik - m_i) comes out times exp(e_ik), |e_ik| <= r_ik,
      r_ik = D_ik + u |s_ik - m_i|                     the exponential's argument, one subtraction (an error of m itself
                                                       moves numerator and denominator alike and cancels)
                  + 2 u                                the exponential: 1 ulp (v_exp_f32; expf in attention.hip)
                  + u (m_i - min_k s_ik) + 2 u T       the online-softmax factors exp(m_old - m_new), T = ceil(L / 64) of them:
                                                       their arguments telescope to at most the row's score range
    it moves numerator and denominator: with e1 = expm1(r), rho_i = sum_k p_ik e1_ik,
      softmax share  = (sum_k p_ik e1_ik |v_kd| + rho_i N_id) / (1 - rho_i)     (no first-order shortcut: rho_i >= 1/2 -> unbounded)
    capped by max_k v_kd - min_k v_kd: whatever the weights, the result stays a convex combination of the window's V rows.  The
    cap is what makes D6b sharp (V constant: the softmax share is 0) and keeps the bound true where the scores are so large
    that fp32 cannot resolve the softmax (the loud windows of D4).
  output error = softmax share
      + (L + 8) u N          fp32 accumulation of P.V over L keys, as _gemm_cases.py counts it
      + (18 T + 2) u N       the row sum: per tile 16 in-lane adds, the rescale and the add of the tile's sum; two cross-lane adds
      + 2 T u N              the rescale of O and of l by the online-softmax factor, one rounding each per tile
      + operands of P.V      f32, f32s: nothing (P is split exactly)
                             fp16 forms: 2^-21 N for P (two-term, p' = 2^14 p; the planes kernel's further 2^(a[k] - A) is an
                             exact power of two) + 2^-21 N for V, and the floors:
                               P: 2^-38 sum_k |v_kd| / l_i                       (f32h_split: p' on the fp16 subnormal grid)
                                  2^-38 sum_k |v_kd| 2^(A - a[k]) / l_i          (planes: a[k] = floor(log2 amax(v_k)), A = max_k a[k];
                                                                                  an all-zero row packs with scale 1: a[k] = 14)
                               V: 2^-38 amax_w  /  2^-38 sum_k p_ik amax(v_k)    (window scale / (row, head) scale)
      + 2 u |out|            1 / l (or scale / l) and the final product
The constants count the operations of the kernels; none is chosen to make a run pass.  test_attention_bounds_host.py shows that
an ideal kernel stays a factor 4 inside the accumulation / operand share of it (bound_acc), as test_gemm_bounds_host.py does for
the contractions; the single roundings enter at face value.
"""
from __future__ import annotations

import functools

import torch

from testkit import mx_emulation as emu

U = 2.0 ** -24
PATTERN = 0x7FA5C3C3            # what every output band holds: a NaN as fp32, so an element nobody stored is not finite
GUARD_ROWS = 256                # rows of band before and after every 2-D buffer
SCALE = 0.125
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
EPS_EXP = 2 * U

FORMS = ("f32", "f32s", "f32h_split", "planes")
PLANES_SCHEDULES = ((1, 1), (1, 0), (2, 0))          # (queries blocks per wavefront, prefetch); (1, 1) is the shipped form
LENGTHS = (1, 16, 17, 63, 64, 65, 127, 128, 129, 399, 798)
SUB_LENGTHS = (17, 65, 129, 399)

SHAPES = {
    "S1": dict(B=1, h=1, Htot=4, heads=[3]),                       # one (window, head) pair: 7 of 8 planes-grid slots exit early
    "S2": dict(B=3, h=5, Htot=16, heads=[13, 1, 7, 4, 12]),        # B h = 15, unsorted heads
    "S3": dict(B=1, h=16, Htot=16, heads=list(range(16))),         # dense, B h = 16
    "S4": dict(B=9, h=1, Htot=12, heads=[11]),                     # B h = 9: just over one XCD round
    "S5": dict(B=2, h=4, Htot=0, heads=None),                      # no bias: the Conformer MHSA
    "S5b": dict(B=3, h=2, Htot=0, heads=None),
    "S6": dict(B=150, h=1, Htot=0, heads=None),                    # many grid rounds, a partial tile in every window (L = 65)
}
CLASSES = ("D1", "D2g", "D2s", "D3", "D4", "D5", "D6a", "D6b")


def has_bias(shape):
    return SHAPES[shape]["heads"] is not None


def cases():
    """[(shape, L, class, strided)] in the order the matrix runs them"""
    out = []
    for L in LENGTHS:
        out += [("S2", L, "D1", False), ("S5", L, "D1", False)]
    for s in ("S1", "S3", "S4", "S5b"):
        out += [(s, L, "D1", False) for L in SUB_LENGTHS]
    out.append(("S6", 65, "D1", False))
    out += [("S2", L, "D1", True) for L in (65, 399)]
    for L in (129, 399, 798):
        out += [(s, L, c, False) for s in ("S2", "S5") for c in ("D2g", "D2s")]
    for L in SUB_LENGTHS:
        out += [(s, L, c, False) for s in ("S2", "S5") for c in ("D3", "D4")]
        out.append(("S2", L, "D5", False))
    out += [("S4", 65, "D4", False), ("S3", 65, "D5", False)]
    for L in (17, 65, 129):
        out += [(s, L, c, False) for s in ("S2", "S5") for c in ("D6a", "D6b")]
    return out


def strides(shape, strided):
    h = SHAPES[shape]["h"]
    return (3 * h * 64 + 8, h * 64 + 5) if strided else (3 * h * 64, h * 64)


def _gen(cls, L, shape):
    return torch.Generator().manual_seed(7919 * CLASSES.index(cls) + 104729 * list(SHAPES).index(shape) + L + 1)


def _d2(g, B, L, h, growing):
    """peaked scores with a planted maximum in every 64-key tile: per (window, head) a unit direction c; the key at a random
    position of tile t is A_t c with A_t growing from 1 towards 2 (the key norms grow with the key index; `growing` False: the
    key order reversed, so they shrink); every other key and the rest of every query are orthogonal to c and small, q.c in
    [0.75, 1.5].  Then q is rescaled so that the float64 scores have std 8."""
    nkt = (L + 63) // 64
    c = torch.randn(B, 1, h, 64, generator=g, dtype=torch.float64)
    c = c / c.norm(dim=-1, keepdim=True)

    def orth(x):
        return x - (x * c).sum(-1, keepdim=True) * c
    k = orth(torch.randn(B, L, h, 64, generator=g, dtype=torch.float64) / 8.0) * torch.linspace(0.5, 1.0, L)[None, :, None, None]
    for t in range(nkt):
        n = min(64, L - 64 * t)
        pos = 64 * t + torch.randint(0, n, (B, h), generator=g)
        for b in range(B):
            for j in range(h):
                k[b, pos[b, j], j] = (1.0 + t / nkt) * c[b, 0, j]
    if not growing:
        k = k.flip(1)
    beta = 0.75 + 0.75 * torch.rand(B, L, h, 1, generator=g, dtype=torch.float64)
    q = beta * c + 0.02 * orth(torch.randn(B, L, h, 64, generator=g, dtype=torch.float64))
    s = SCALE * torch.einsum("bihd,bkhd->bhik", q, k)
    q = q * (8.0 / float(s.std()))
    v = torch.randn(B, L, h, 64, generator=g, dtype=torch.float64)
    return torch.cat([q.reshape(B * L, -1), k.reshape(B * L, -1), v.reshape(B * L, -1)], 1).float()


@functools.lru_cache(maxsize=4)
def make_inputs(shape, L, cls):
    """dict(qkv f32 [B L, 3 h 64] = [q heads | k heads | v heads], gate f32 [B L, Htot] / None, table f32 [Htot, 2 L - 1] / None,
    heads, amax f32 [B]: the per-window |max| of qkv as the entry points compute it)"""
    sh = SHAPES[shape]
    B, h, Htot, heads = sh["B"], sh["h"], sh["Htot"], sh["heads"]
    g = _gen(cls, L, shape)
    qkv = torch.randn(B * L, 3 * h * 64, generator=g)
    gate = table = None
    if heads is not None:
        gate = torch.rand(B * L, Htot, generator=g) * 2
        table = torch.randn(Htot, 2 * L - 1, generator=g)
    if cls in ("D2g", "D2s"):
        assert L >= 129
        qkv = _d2(g, B, L, h, cls == "D2g")
        if table is not None:
            table = table * 0.05             # the planted maxima, not the bias, decide
    elif cls == "D3":
        mag = torch.exp2(torch.randint(-9, 10, (B * L, 2 * h), generator=g).float())
        qkv[:, h * 64:] = (qkv[:, h * 64:].view(B * L, 2 * h, 64) * mag[..., None]).view(B * L, 2 * h * 64)
        qkv[:, :h * 64] *= 0.05
    elif cls == "D4":
        assert L % 64 != 0
        w = torch.tensor([2.0 ** -12, 2.0 ** 8])[torch.arange(B) % 2]
        qkv = (qkv.view(B, L, -1) * w[:, None, None]).view(B * L, -1)
    elif cls == "D5":
        assert heads is not None
        table = torch.rand(Htot, 2 * L - 1, generator=g) * 60 - 30
    elif cls == "D6a":
        assert B >= 2
        qkv.view(B, L, -1)[0] = 0.0
    elif cls == "D6b":
        vec = torch.randn(B, 1, h * 64, generator=g)
        qkv.view(B, L, -1)[:, :, 2 * h * 64:] = vec
    qkv = qkv.contiguous()
    amax = qkv.view(B, -1).abs().amax(1).float()
    return dict(qkv=qkv, gate=gate, table=table, heads=heads, amax=amax, B=B, L=L, h=h, Htot=Htot)


def split_qkv(qkv, B, L, h):
    """q, k, v as [B, h, L, 64] views"""
    return [qkv[:, i * h * 64:(i + 1) * h * 64].view(B, L, h, 64).permute(0, 2, 1, 3) for i in range(3)]


def bias_of(gate_w, table, heads, L):
    """float64 [h, L, L]: gate[i, H] table[H, k - i + L - 1] of one window (gate_w [L, Htot])"""
    idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
    return gate_w.double()[:, heads].T[:, :, None] * table.double()[heads][:, idx]


def _attn_ref(q, k, v, bias=None):
    """the float64 softmax attention (test_ops_gpu.py's _attn_ref) with the intermediates the bound needs"""
    s = (q.double() * SCALE) @ k.double().transpose(-1, -2)
    if bias is not None:
        s = s + bias.double()
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    return dict(s=s, m=m, l=l, p=p, out=p @ v.double(), N=p @ v.double().abs(),
                S1=SCALE * (q.double().abs() @ k.double().abs().transpose(-1, -2)), gT=None if bias is None else bias.double().abs())


def v_exponent(row_amax):
    """a[k] of attention_planes.hip: floor(log2 |max| of the V row); an all-zero row packs with scale 1, which reads as 14"""
    safe = row_amax.clamp_min(1e-300)
    return torch.where(row_amax > 0, torch.floor(torch.log2(safe)), torch.full_like(row_amax, 14.0))


def _softmax_share(p, r, vabs, N, hull):
    e1 = torch.expm1(r)
    pe = p * e1
    rho = pe.sum(-1, keepdim=True)
    sm = (pe @ vabs + rho * N) / (1.0 - rho).clamp_min(0.5)
    sm = torch.where(rho < 0.5, sm, torch.full_like(sm, float("inf")))
    return torch.minimum(sm, hull)


def window_bound(form, ref, q, k, v, amax_w, L):
    """(bound, bound_acc) [h, L, 64] of one window: q, k, v [h, L, 64], ref = _attn_ref of them, amax_w the window's |max|.
    bound_acc: the share that descends from accumulation order and operand splitting (what the factor 4 is asked of)."""
    q, k, v = q.double(), k.double(), v.double()
    nkt = (L + 63) // 64
    s, m, p, N, S1, l = ref["s"], ref["m"], ref["p"], ref["N"], ref["S1"], ref["l"]
    vabs = v.abs()
    hull = v.amax(1, keepdim=True) - v.amin(1, keepdim=True)                   # [h, 1, 64]
    r_rnd = U * (s - m).abs() + EPS_EXP + U * (m - s.amin(-1, keepdim=True)) + nkt * EPS_EXP
    if ref["gT"] is not None:
        r_rnd = r_rnd + 3 * U * ref["gT"] + U * s.abs()
    d_acc = (64 + 8 + 2) * U * S1
    o_rnd = 2 * U * ref["out"].abs()
    o_acc = ((L + 8) + (18 * nkt + 2) + 2 * nkt) * U * N
    aw = float(amax_w)
    ksum = k.abs().sum(-1)[:, None, :]                     # [h, 1, L]  sum_d |k_kd|
    qsum = SCALE * q.abs().sum(-1)[:, :, None]             # [h, L, 1]
    if form == "f32h_split":
        d_acc = d_acc + 2.0 ** -21 * S1 + 2.0 ** -38 * aw * (ksum + qsum)
        o_acc = o_acc + 2 * 2.0 ** -21 * N + 2.0 ** -38 * vabs.sum(1, keepdim=True) / l + 2.0 ** -38 * aw
    elif form == "planes":
        ka, va = k.abs().amax(-1), v.abs().amax(-1)        # [h, L]: the (row, head) maxima
        d_acc = d_acc + 2.0 ** -21 * S1 + 2.0 ** -38 * (aw * ksum + ka[:, None, :] * qsum)
        a = v_exponent(va)
        w = torch.exp2(a.amax(-1, keepdim=True) - a)       # 2^(A - a[k])
        o_acc = o_acc + 2 * 2.0 ** -21 * N + 2.0 ** -38 * (vabs * w[..., None]).sum(1, keepdim=True) / l + 2.0 ** -38 * (p @ va[..., None])
    else:
        assert form in ("f32", "f32s")
    e_rnd = _softmax_share(p, r_rnd, vabs, N, hull) + o_rnd
    e_all = _softmax_share(p, r_rnd + d_acc, vabs, N, hull) + o_rnd + o_acc
    return e_all, (e_all - e_rnd).clamp_min(0.0)


def _bound_key(form):
    return "f32" if form in ("f32", "f32s") else form


@functools.lru_cache(maxsize=3)
def launch_ref(shape, L, cls):
    """float64 reference and bounds of a whole launch: dict(out [B L, h 64], bound / bound_acc {f32, f32h_split, planes: [B L, h
    64]}, windows: per window the input conditions the classes claim (pmax [h, L], argmax of s and of q.k, tile maxima))"""
    inp = make_inputs(shape, L, cls)
    B, h, heads = inp["B"], inp["h"], inp["heads"]
    q, k, v = split_qkv(inp["qkv"], B, L, h)
    out = torch.zeros(B, L, h * 64, dtype=torch.float64)
    bound = {f: torch.zeros(B, L, h * 64, dtype=torch.float64) for f in ("f32", "f32h_split", "planes")}
    bacc = {f: torch.zeros(B, L, h * 64, dtype=torch.float64) for f in bound}
    windows = []
    for b in range(B):
        bias = bias_of(inp["gate"].view(B, L, -1)[b], inp["table"], heads, L) if heads is not None else None
        ref = _attn_ref(q[b], k[b], v[b], bias)
        out[b] = ref["out"].permute(1, 0, 2).reshape(L, h * 64)
        for f in bound:
            e, ea = window_bound(f, ref, q[b], k[b], v[b], inp["amax"][b], L)
            bound[f][b] = e.permute(1, 0, 2).reshape(L, h * 64)
            bacc[f][b] = ea.permute(1, 0, 2).reshape(L, h * 64)
        s_qk = ref["s"] if bias is None else ref["s"] - bias
        tiles = torch.stack([ref["s"][..., t:t + 64].amax(-1) for t in range(0, L, 64)], -1)      # [h, L, nkt]
        windows.append(dict(pmax=ref["p"].amax(-1), arg_s=ref["s"].argmax(-1), arg_qk=s_qk.argmax(-1), tile_max=tiles))
    return dict(out=out.view(B * L, h * 64), bound={f: x.view(B * L, h * 64) for f, x in bound.items()},
                bound_acc={f: x.view(B * L, h * 64) for f, x in bacc.items()}, windows=windows)


def bound_of(ref, form):
    return ref["bound"][_bound_key(form)], ref["bound_acc"][_bound_key(form)]


# ---- an ideal kernel on the CPU: the form's operand rounding, fp32 accumulation in a stated order, an fp32 softmax ----
def _f32(x):
    return x.float().double()


def _acc(acc, terms, order, block):
    """acc [.., M, N] fp32-valued float64 += sum over the last dim of a and the matching dim of b for every (a [.., M, K], b [.., N,
    K]) in terms; "forward": one rounding per product; "blocked": per term the exact sum of `block` products, rounded, then added"""
    K = terms[0][0].shape[-1]
    step = 1 if order == "forward" else block
    for k0 in range(0, K, step):
        for a, b in terms:
            if step == 1:
                acc = _f32(acc + a[..., :, None, k0] * b[..., None, :, k0])
            else:
                acc = _f32(acc + a[..., k0:k0 + step] @ b[..., k0:k0 + step].transpose(-1, -2))
    return acc


def _operand_terms(form, a, b, sa, sb, single=False):
    """products the form's kernel adds up for a . b, smallest first; sa / sb: the fp16 scales (float64, broadcastable)"""
    if form == "f32":
        return [(a, b)]
    if form == "f32s":
        ah, am, al = emu.bf16x3_terms(a.float())
        bh, bm, bl = emu.bf16x3_terms(b.float())
        return [(al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh)]
    ah, al = emu.h2_terms(a.float(), sa)
    bh, bl = emu.h2_terms(b.float(), sb)
    return [(ah, bh)] if single else [(al, bh), (ah, bl), (ah, bh)]


def ideal_window(form, q, k, v, gate_h, table_h, amax_w, L, order, fault=None):
    """one window of an ideal kernel of `form`: q, k, v f32 [h, L, 64]; gate_h f32 [h, L] / None (the gate of each kept head),
    table_h f32 [h, 2 L - 1]; order "forward" (one softmax over the row, P.V key by key) or "blocked" (online softmax over 64-key
    tiles, P.V by 16 keys).  Returns f32-valued float64 [h, L, 64].
    fault: a subtly WRONG kernel, for test_attention_bounds_host.py's proof that the net catches it: "leak" (one masked key of a
    partial last tile, score 0, counted into the row sum), "norescale" (blocked order: O misses the online-softmax factor of the
    last tile), "single" (fp16 forms: the hi terms only)."""
    log2 = form != "f32"
    c = float(torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E_F32 if log2 else 1.0, dtype=torch.float32))
    qs = _f32(q.double() * c)
    sw = emu._pow2_scale_h2(torch.as_tensor(float(amax_w), dtype=torch.float64)) if float(amax_w) > 0 else torch.tensor(1.0, dtype=torch.float64)
    kd, vd = k.double(), v.double()
    if form == "planes":
        ka, va = k.abs().amax(-1, keepdim=True).double(), v.abs().amax(-1, keepdim=True).double()
        sk = torch.where(ka > 0, emu._pow2_scale_h2(ka), torch.ones_like(ka))
        sv = torch.where(va > 0, emu._pow2_scale_h2(va), torch.ones_like(va))
        a_k = v_exponent(va)[..., 0]                        # [h, L]
    else:
        sk = sv = sw
    t = _acc(torch.zeros(q.shape[0], L, L, dtype=torch.float64), _operand_terms(form, qs, kd, sw, sk, fault == "single"), order, 4)
    if gate_h is not None:
        idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1
        g = _f32(gate_h.double() * (LOG2E_F32 if log2 else 1.0))
        t = _f32(t + g[:, :, None] * table_h.double()[:, idx])
    ex = (lambda x: _f32(torch.exp2(x))) if log2 else (lambda x: _f32(torch.exp(x)))
    h = q.shape[0]
    O = torch.zeros(h, L, 64, dtype=torch.float64)
    l = torch.zeros(h, L, 1, dtype=torch.float64)

    def pv_terms(p, k0, k1, A):
        """P.V operand terms for keys k0 .. k1: p [h, L, n] un-normalised probabilities, V rows transposed to [h, 64, n]"""
        vt = vd[:, k0:k1].transpose(-1, -2)
        if form in ("f32", "f32s"):
            return _operand_terms(form, p, vt, None, None)
        if form == "planes":
            ps = torch.exp2(14.0 + a_k[:, None, k0:k1] - A)                    # p' = 2^14 p 2^(a[k] - A)
            return _operand_terms(form, p, vt, ps, sv[:, k0:k1].transpose(-1, -2), fault == "single")
        return _operand_terms(form, p, vt, torch.tensor(2.0 ** 14, dtype=torch.float64), sw, fault == "single")

    if order == "forward":
        m = t.amax(-1, keepdim=True)
        p = ex(_f32(t - m))
        for kk in range(L):
            l = _f32(l + p[..., kk:kk + 1])
        A = a_k.amax(-1)[:, None, None] if form == "planes" else None
        O = _acc(O, pv_terms(p, 0, L, A), "forward", 1)
    else:
        m = torch.full((h, L, 1), -float("inf"), dtype=torch.float64)
        A = torch.full((h, 1, 1), -126.0, dtype=torch.float64)
        for k0 in range(0, L, 64):
            k1 = min(k0 + 64, L)
            m_new = torch.maximum(m, t[..., k0:k1].amax(-1, keepdim=True))
            alpha = ex(_f32(m - m_new))
            p = ex(_f32(t[..., k0:k1] - m_new))
            psum = torch.zeros_like(l)
            for j in range(0, k1 - k0, 16):
                psum = _f32(psum + _f32(p[..., j:j + 16].sum(-1, keepdim=True)))
            l = _f32(_f32(l * alpha) + psum)
            if not (fault == "norescale" and k1 == L):
                O = _f32(O * alpha)
            if form == "planes":
                A = torch.maximum(A, a_k[:, k0:k1].amax(-1)[:, None, None])
            O = _acc(O, pv_terms(p, k0, k1, A), "blocked", 16)
            m = m_new
    if fault == "leak" and L % 64:
        l = _f32(l + ex(_f32(0.0 - m)))
    return _f32(O * _f32(1.0 / l))
