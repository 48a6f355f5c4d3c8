"""csrc/posconv_resident.hip — the positional conv on resident plane rows — at two levels.

Op level (ops.posconv on the planes of ops.pad_rows_split2): against (i) the generic pre-split contraction on the same
descriptor, byte for byte, and (ii) the float64 conv within the bound _gemm_cases.py derives for an fp16-pair (f32h) contraction
of that K followed by bias, GELU and the residual.  256-row flat tiles: the L list puts a window boundary inside a tile
(B = 3), several inside one (L = 1, 15), a ragged last tile, and exactly one tile either side of 128 / 256 rows.

Engine level: Engine.segment on tiny_ln (taps 16, groups 4, cg 64) and on the same model with 128 taps, against an engine
created under DZN_NO_POSCONV_RESIDENT=1, byte for byte, with the profiler saying which kernel each of them ran.
"""
import os
from dataclasses import replace

import pytest
import torch

import _gemm_cases as gc
from diarizen_amd import _lib

pytestmark = pytest.mark.gpu

LS = (1, 15, 79, 80, 81, 127, 128, 129, 399)
BS = (1, 3)
GELU = _lib.DZN_ACT_GELU


def _inputs(B, L, taps, G, cg, seed, zero_first=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * L, G * cg, generator=g)
    x *= torch.exp2(torch.randint(-3, 4, (B * L, 1), generator=g).float())     # rows of different magnitude inside a window
    if zero_first:
        x[:L] = 0.0
    W = torch.zeros(G * cg, taps, 64)
    W[:, :, :cg] = torch.randn(G * cg, taps, cg, generator=g) / (taps * cg) ** 0.5
    bias = 0.1 * torch.randn(G * cg, generator=g)
    return x, W.reshape(G * cg, taps * 64).contiguous(), bias


def _run(ops, dev, x, W, bias, B, L, taps, G, cg, resident, h2w=None):
    """(out, tracker of out per window, snapshot): x + gelu(conv(x) + bias), as the engine launches it"""
    xd, Wd, bd = x.to(dev), W.to(dev), bias.to(dev)
    amax = x.view(B, -1).abs().amax(1).to(dev)
    planes, snap = ops.pad_rows_split2(xd, amax, B=B, L=L, taps=taps, G=G, cg=cg)
    h2w = h2w or ops.split_weights_h2(Wd)
    c_amax = torch.zeros(B, device=dev)
    out = torch.full((B * L, G * cg), float("nan"), device=dev)
    ops.posconv(planes, snap, Wd, h2w, B=B, L=L, taps=taps, G=G, cg=cg, bias=bd, R=xd, out=out, act=GELU, c_amax=c_amax,
                resident=resident)
    torch.cuda.synchronize()
    return out.cpu(), c_amax.cpu(), snap.cpu()


def _reference(x, W, bias, B, L, taps, G, cg):
    """float64 x + gelu(conv + bias) and its bound (gc.product_ref "f32h" per group on the im2col rows, then gc.epilogue_ref)"""
    pad = taps // 2
    xp = torch.zeros(B, L + taps, G, 64)
    xp[:, pad:pad + L, :, :cg] = x.view(B, L, G, cg)
    row_amax = x.view(B, -1).abs().amax(1).repeat_interleave(L)[:, None]
    C, E = torch.empty(B * L, G * cg, dtype=torch.float64), torch.empty(B * L, G * cg, dtype=torch.float64)
    for g in range(G):
        A = xp[:, :, g, :].unfold(1, taps, 1)[:, :L]                    # [B, L, 64, taps]
        A = A.permute(0, 1, 3, 2).reshape(B * L, taps * 64).contiguous()
        cols = slice(g * cg, (g + 1) * cg)
        P, e, _ = gc.product_ref("f32h", A, row_amax, W[cols])
        c, ec, _ = gc.epilogue_ref(P, e, bias=bias[cols], act=GELU, R=x[:, cols])
        C[:, cols], E[:, cols] = c, ec
    return C, E


def _check(ops, dev, B, L, taps, G, cg, seed, zero_first=False):
    assert ops.posconv_resident_fits(B, L, taps)
    x, W, bias = _inputs(B, L, taps, G, cg, seed, zero_first)
    res, res_amax, snap = _run(ops, dev, x, W, bias, B, L, taps, G, cg, True)
    gen, gen_amax, _ = _run(ops, dev, x, W, bias, B, L, taps, G, cg, False)
    assert torch.isfinite(res).all()
    assert torch.equal(res.view(torch.int32), gen.view(torch.int32))
    assert torch.equal(res_amax, gen_amax) and torch.equal(res_amax, res.view(B, -1).abs().amax(1))
    if zero_first:
        assert float(snap[0]) == 0.0
    ref, bound = _reference(x, W, bias, B, L, taps, G, cg)
    ratio = ((res.double() - ref).abs() / bound).max().item()
    print(f"[posconv resident] B={B} L={L} taps={taps} G={G} cg={cg}: max |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("L", LS)
def test_op_equals_generic_kernel_and_float64(built_lib, gpu, L, B):
    from diarizen_amd import ops
    _check(ops, gpu, B, L, 16, 4, 64, 1000 * L + B)


def test_op_first_window_all_zero(built_lib, gpu):
    """window 0 is zeros: its tracker is 0, the zero case of h2_scale (scale 1); its rows share a tile with window 1's"""
    from diarizen_amd import ops
    _check(ops, gpu, 3, 81, 16, 4, 64, 7, zero_first=True)


def test_op_padded_groups(built_lib, gpu):
    """the base models' groups: 48 channels in planes of 64, N = 48 columns of a 64-column tile"""
    from diarizen_amd import ops
    _check(ops, gpu, 3, 81, 16, 4, 48, 8)


def test_op_128_taps(built_lib, gpu):
    """the model's tap count at B = 2: 511 resident rows, a window boundary inside the first tile, a ragged second tile"""
    from diarizen_amd import ops
    _check(ops, gpu, 2, 129, 128, 2, 64, 9)


def test_op_more_items_than_resident_workgroups(built_lib, gpu):
    """19 row tiles x 16 groups = 304 workgroups of ~98 KB of LDS (one per CU) on 256 CUs"""
    from diarizen_amd import ops
    _check(ops, gpu, 12, 399, 16, 16, 64, 10)


def test_op_refuses_a_span_that_does_not_fit(built_lib, gpu):
    """L = 1 at B = 200: 199 window gaps inside one tile; the generic kernel keeps such shapes (no launch, DZN_E_INVALID)"""
    from diarizen_amd import ops
    B, L, taps, G, cg = 200, 1, 16, 4, 64
    assert not ops.posconv_resident_fits(B, L, taps)
    x, W, bias = _inputs(B, L, taps, G, cg, 11)
    with pytest.raises(_lib.DznError):
        _run(ops, gpu, x, W, bias, B, L, taps, G, cg, True)
    gen, _, _ = _run(ops, gpu, x, W, bias, B, L, taps, G, cg, False)
    assert torch.isfinite(gen).all()


def test_poisoned_window_stays_in_its_window(built_lib, gpu):
    """NaN in window 1 of 3 (its tracker too): windows 0 and 2 — whose rows share 256-row tiles with window 1's — are the bits
    of a clean call, because the zero gap rows of the padded copy isolate the windows"""
    from diarizen_amd import ops
    B, L, taps, G, cg = 3, 129, 16, 4, 64
    x, W, bias = _inputs(B, L, taps, G, cg, 12)
    clean, clean_amax, _ = _run(ops, gpu, x, W, bias, B, L, taps, G, cg, True)
    xn = x.clone()
    xn[L:2 * L] = float("nan")
    bad, bad_amax, _ = _run(ops, gpu, xn, W, bias, B, L, taps, G, cg, True)
    assert torch.isnan(bad[L:2 * L]).all()
    for w in (0, 2):
        rows = slice(w * L, (w + 1) * L)
        assert torch.equal(bad[rows].view(torch.int32), clean[rows].view(torch.int32))
        assert torch.equal(bad_amax[w], clean_amax[w])


# ---- engine level ----
ENGINE_B = 3
ENGINE_LS = (1, 15, 81, 129, 399)


def _samples(cfg, L):
    n = 400
    while cfg.num_frames(n) < L:
        n += 160
    assert cfg.num_frames(n) == L
    return n


def _engine_pair(cfg, gpu, B, Ls, seed):
    """{L: {"default" | "off": (logp, multilabel, launches per class)}}; "off" = an engine created under DZN_NO_POSCONV_RESIDENT=1"""
    from diarizen_amd.engine import Engine
    from oracle import seg_model
    from oracle.gen_golden import synth_wave
    sd = seg_model.seg_state_dict(cfg, 0)
    ns = {L: _samples(cfg, L) for L in Ls}
    out = {L: {} for L in Ls}
    for key, off in (("default", False), ("off", True)):
        old = os.environ.pop("DZN_NO_POSCONV_RESIDENT", None)
        if off:
            os.environ["DZN_NO_POSCONV_RESIDENT"] = "1"
        try:
            eng = Engine(cfg, sd, max_batch=B, max_samples=max(ns.values()), precision="f32h", device=gpu)
        finally:
            os.environ.pop("DZN_NO_POSCONV_RESIDENT", None)
            if old is not None:
                os.environ["DZN_NO_POSCONV_RESIDENT"] = old
        for L in Ls:
            w = synth_wave(B, ns[L], seed + L).to(gpu)
            _lib.profile_enable(True)
            try:
                logp, ml = eng.segment(w)
                torch.cuda.synchronize()
                launches = {p["name"]: p["launches"] for p in _lib.profile_collect()}
            finally:
                _lib.profile_enable(False)
            out[L][key] = (logp.cpu(), ml.cpu(), launches)
        eng.close()
    return out


def _assert_pair(pair, L):
    (logp, ml, ran), (logp0, ml0, ran0) = pair["default"], pair["off"]
    assert logp.shape[1] == L and torch.isfinite(logp).all()
    assert torch.equal(logp.view(torch.int32), logp0.view(torch.int32)) and torch.equal(ml, ml0)
    assert ran.get("posconv_f32h", 0) == 1 and "gemm_f32h_pre_128x64" not in ran, ran
    assert ran0.get("gemm_f32h_pre_128x64", 0) == 1 and "posconv_f32h" not in ran0, ran0


@pytest.fixture(scope="module")
def tiny_pairs(built_lib, gpu):
    from diarizen_amd.configs import TINY_LN
    return _engine_pair(TINY_LN, gpu, ENGINE_B, ENGINE_LS, 20)


@pytest.mark.parametrize("L", ENGINE_LS)
def test_engine_equals_the_engine_without_the_resident_kernel(tiny_pairs, L):
    _assert_pair(tiny_pairs[L], L)


def test_engine_128_taps(built_lib, gpu):
    from diarizen_amd.configs import TINY_LN
    cfg = replace(TINY_LN, name="tiny_ln_taps128", pos_conv_kernel=128)
    _assert_pair(_engine_pair(cfg, gpu, 2, (129,), 30)[129], 129)
