"""dzn_embed_forward_strided (windows read through a strided view of one recording; the fbank computed once per recording
frame where the stride allows it) against dzn_embed_forward on the dense copy of the same windows.

Everything in front of the per-window mean is per frame and the contractions are row-independent, so the claim is
BIT identity: the `fbank` debug tap and the embeddings are compared with array_equal / torch.equal, no tolerance.
Shapes: N = 2000 (T = 11 frames) is the smallest window with several frames per stride; the engine's fbank pass holds
(124 - 1) * 2 + 11 = 257 rows, so the cases below also cross the pass boundary on both paths."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SMALL, B_MAX, L_MASK = 2000, 124, 5


def _make_engine(gpu, B, N, taps):
    import os
    from diarizen_amd.configs import RESNET34, get_seg_config
    from diarizen_amd.engine import Engine
    from oracle import emb_model, seg_model
    cfg = get_seg_config("tiny_ln")
    if taps:
        os.environ["DZN_DEBUG_TAPS"] = "1"
    try:
        return Engine(cfg, seg_model.seg_state_dict(cfg, 0), RESNET34, emb_model.emb_state_dict(0),
                      max_batch=B, max_samples=N, precision="f32h", device=gpu)
    finally:
        os.environ.pop("DZN_DEBUG_TAPS", None)


@pytest.fixture(scope="module")
def eng_taps(built_lib, gpu):
    e = _make_engine(gpu, B_MAX, N_SMALL, taps=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_plain(built_lib, gpu):
    e = _make_engine(gpu, B_MAX, N_SMALL, taps=False)
    yield e
    e.close()


def _recording(gpu, B, N, stride, seed):
    """seeded noise + a chirp-like tone, (B - 1) * stride + N samples, and the [B, N] view of its windows"""
    n = (B - 1) * stride + N
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32)
    rec = 0.05 * torch.randn(n, generator=g) + 0.2 * torch.sin(t * (0.05 + 0.25 * t / n))
    rec = (rec * (0.3 + 0.7 * torch.rand(n, generator=g).cumsum(0) / n)).to(gpu)
    return rec, torch.as_strided(rec, (B, N), (stride, 1))


def _masks(gpu, B, seed, L=L_MASK):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, 4, L, generator=g) > 0.4).float()
    m[:, 0, 0] = 1.0                     # every window has an active speaker
    return m.to(gpu)


def _both(eng, views, masks, taps):
    """(embeddings, fbank tap) of the strided entry and of the dense entry on the contiguous copy"""
    a = eng.embed_strided(views, masks).clone()
    torch.cuda.synchronize()
    fa = eng.debug_fetch("fbank").copy() if taps else None
    b = eng.embed(views.contiguous(), masks).clone()
    torch.cuda.synchronize()
    fb = eng.debug_fetch("fbank").copy() if taps else None
    return a, fa, b, fb


# shared strides 160 / 320 / 800 / 1760 (= N - 400 + 160, the largest without a gap); 2000 (= N: gaps) and 801 (no
# multiple of the shift) fall back to the per-window arithmetic read at the stride
STRIDES = [160, 320, 800, 1760, 2000, 801]
# (B, stride) with G = (B - 1) q + 11 at the row-tile edges of the fp32 contraction: 128, 129, 257; and G = 1364 in
# several passes of the 257-row workspace
EDGES = [(118, 160), (60, 320), (124, 320), (124, 1760)]


@pytest.mark.parametrize("B,stride", [(B, s) for s in STRIDES for B in (1, 2, 11)] + EDGES)
def test_strided_entry_equals_dense_entry_bit_for_bit(eng_taps, gpu, B, stride):
    from diarizen_amd.inference import fbank_grid, fbank_is_shared
    if (B, stride) in EDGES:
        assert fbank_grid(B, N_SMALL, stride)[2] == {(118, 160): 128, (60, 320): 129, (124, 320): 257, (124, 1760): 1364}[(B, stride)]
    assert fbank_is_shared(N_SMALL, stride) == (stride in (160, 320, 800, 1760))
    rec, views = _recording(gpu, B, N_SMALL, stride, seed=1000 + stride + B)
    masks = _masks(gpu, B, seed=B)
    a, fa, b, fb = _both(eng_taps, views, masks, taps=True)
    assert fa.shape == fb.shape == (B * 11 * 80,)
    assert np.isfinite(fb).all() and np.abs(fb).max() > 0.1
    assert np.array_equal(fa, fb), f"fbank differs in {(fa != fb).sum()} of {fa.size} values, max |d| {np.abs(fa - fb).max()}"
    assert torch.equal(a, b), f"embeddings differ: max |d| {(a - b).abs().max().item()}"


def test_real_geometry(built_lib, gpu):
    """8 s windows 0.8 s apart: N = 128000, stride 12800 (q = 80, T = 798), B = 3"""
    B, N, stride = 3, 128000, 12800
    eng = _make_engine(gpu, B, N, taps=True)
    rec, views = _recording(gpu, B, N, stride, seed=7)
    a, fa, b, fb = _both(eng, views, _masks(gpu, B, seed=8, L=399), taps=True)
    eng.close()
    assert fa.shape == (B * 798 * 80,)
    assert np.array_equal(fa, fb)
    assert torch.equal(a, b)


def test_silent_windows_first_middle_last(eng_plain, gpu):
    """the trunk subset (windows without an active speaker skip the ResNet) meets the shared fbank: same bits as the dense
    entry, the silent windows are seg_1's bias, and both calls counted them"""
    from oracle import emb_model
    B, stride = 11, 800
    rec, views = _recording(gpu, B, N_SMALL, stride, seed=21)
    masks = _masks(gpu, B, seed=22)
    silent = [0, 5, 10]
    masks[silent] = 0.0
    w0, k0 = eng_plain.embed_skip_stats()
    a, _, b, _ = _both(eng_plain, views, masks, taps=False)
    w1, k1 = eng_plain.embed_skip_stats()
    assert (w1 - w0, k1 - k0) == (2 * B, 2 * len(silent))
    assert torch.equal(a, b)
    bias = emb_model.emb_state_dict(0)["resnet.seg_1.bias"].to(gpu)
    assert torch.equal(a[silent], bias.expand(len(silent), 4, -1))
    assert not torch.equal(a[1, 0], bias)


def test_strided_entry_replays_from_a_hip_graph(eng_plain, gpu):
    """the strided entry only enqueues (no read-back, no allocation, no second stream): it is captured in a HIP graph and the
    replay gives the eager bits of the dense entry, for a new recording written into the same buffer as well"""
    B, stride = 11, 320
    rec, views = _recording(gpu, B, N_SMALL, stride, seed=31)
    masks = _masks(gpu, B, seed=32)
    masks[3] = 0.0
    eager = eng_plain.embed(views.contiguous(), masks).clone()      # also builds the per-geometry tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = eng_plain.embed_strided(views, masks)
    torch.cuda.synchronize()
    for rep in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), f"replay {rep}: max |d| {(out - eager).abs().max().item()}"
    rec2, _ = _recording(gpu, B, N_SMALL, stride, seed=33)
    rec.copy_(rec2)
    eager2 = eng_plain.embed(views.contiguous(), masks).clone()
    torch.cuda.synchronize()
    assert not torch.equal(eager2, eager)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)
