"""The 1x1 stride-2 shortcut of a ResNet down-sampling block folded into conv2 as a second A segment of the contraction
(dzn_gemm_desc.A2): out = relu(conv2(mid) + b2 + Ws x_centre + bs) as ONE sum over K = 9 C + C_prev.

Op level: ops.gemm with the second segment on zero-bordered channels-last images and row tables built as the trunk builds
tab1 / tab2, against torch's float64 convolutions (bar: the op bar of test_ops_gpu.py, 1e-5 of the output's |max|) and against
the three-launch form — shortcut, then conv2 with the shortcut image as residual (bar: 2e-6 of |max|; the two forms round
differently, so bit equality is not asked).  Engine level: two engines in two fresh processes, with and without
DZN_NO_SHORTCUT_FUSION."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = {"f32h": 3, "f32s": 2, "f32": 0}
# (previous C, C, H, W of the output), batch 3: a half-empty last 64-column tile (k2 = 32 after K1 = 576), an exact one,
# a single output pixel, and M = 129 rows per image (the second 128-row tile holds one live row)
GEOMS = {"c32_3x5": (32, 64, 3, 5), "c64_2x3": (64, 128, 2, 3), "c128_1x1": (128, 256, 1, 1), "m129": (32, 64, 3, 43)}
B = 3
_CASES = {}


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / (b.double().abs().max().item() + 1e-300)


def _case(name, prev_gain=1.0, mid_gain=1.0):
    """images, weights, row tables and the float64 reference of one geometry (host tensors, built once, never modified)"""
    key = (name, prev_gain, mid_gain)
    if key in _CASES:
        return _CASES[key]
    Cp, C, H, W = GEOMS[name]
    Hp, Wp = 2 * H - 1, 2 * W          # (Hp - 1) // 2 + 1 == H and (Wp - 1) // 2 + 1 == W: one odd, one even extent
    g = torch.Generator().manual_seed(1000 * Cp + 10 * H + W)
    prev = torch.zeros(B, Hp + 2, Wp + 2, Cp)
    prev[:, 1:-1, 1:-1] = torch.randn(B, Hp, Wp, Cp, generator=g) * prev_gain
    mid = torch.zeros(B, H + 2, W + 2, C)
    mid[:, 1:-1, 1:-1] = torch.randn(B, H, W, C, generator=g).relu() * mid_gain
    w2 = torch.randn(C, C, 3, 3, generator=g) * torch.linspace(0.5, 1.5, C)[:, None, None, None] / (3.0 * C ** 0.5)
    ws = torch.randn(C, Cp, 1, 1, generator=g) * torch.linspace(1.5, 0.5, C)[:, None, None, None] / Cp ** 0.5
    b2, bs = torch.randn(C, generator=g), torch.randn(C, generator=g)
    K1, k2 = 9 * C, Cp
    W2 = w2.permute(0, 2, 3, 1).reshape(C, K1).contiguous()          # k = (dh * 3 + dw) * C + ci
    Ws = ws.reshape(C, Cp).contiguous()
    Wcat = torch.zeros(C, K1 + (k2 + 63) // 64 * 64)
    Wcat[:, :K1] = W2
    Wcat[:, K1:K1 + k2] = Ws
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tab1 = ((ys * (W + 2) + xs) * C).reshape(-1).to(torch.int32)                 # top-left of the 3x3 patch
    tab2 = ((2 * ys * (Wp + 2) + 2 * xs) * Cp).reshape(-1).to(torch.int32)       # top-left of the stride-2 patch
    ref = torch.nn.functional.conv2d(mid[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double(), w2.double(), b2.double(), padding=1)
    ref = ref + torch.nn.functional.conv2d(prev[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double(), ws.double(), bs.double(), stride=2)
    ref = ref.relu().permute(0, 2, 3, 1).contiguous()                            # [B, H, W, C]
    c = dict(Cp=Cp, C=C, H=H, W=W, Hp=Hp, Wp=Wp, K1=K1, k2=k2, prev=prev, mid=mid, W2=W2, Ws=Ws, Wcat=Wcat, b2=b2, bs=bs,
             tab1=tab1, tab2=tab2, ref=ref)
    _CASES[key] = c
    return c


def _amax(img):
    return img.reshape(img.shape[0], -1).abs().amax(dim=1).float().contiguous()


def _fused(c, gpu, prec, prev=None, prev_amax=None, k1=None, precision_kw=None):
    from diarizen_amd import ops
    C, H, W, Cp, Wp = c["C"], c["H"], c["W"], c["Cp"], c["Wp"]
    prev = (c["prev"] if prev is None else prev).to(gpu)
    mid = c["mid"].to(gpu)
    out = torch.zeros_like(mid)
    img, pimg = mid[0].numel(), prev[0].numel()
    interior = ((W + 2) + 1) * C
    centre = ((Wp + 2) + 1) * Cp
    kw = dict(precision_kw or {})
    if prec != 0:
        kw.update(a_amax=_amax(mid), a2_amax=_amax(c["prev"].to(gpu)) if prev_amax is None else prev_amax)
    ops.gemm(mid.reshape(-1), c["Wcat"].to(gpu), M=H * W, N=C, K=c["Wcat"].shape[1], lda=0, a_rowoff=c["tab1"].to(gpu),
             c_rowoff=c["tab1"].to(gpu), kc=3 * C, ldk=(W + 2) * C, bias=(c["b2"] + c["bs"]).to(gpu), post_relu=True, nz=B,
             zs=dict(a_z0=img, c_z0=img), C_out=out.reshape(-1)[interior:], precision=prec, amax_unit=0,
             A2=prev.reshape(-1)[centre:], a2_rowoff=c["tab2"].to(gpu), a2_z0=pimg, k1=c["K1"] if k1 is None else k1,
             k2=c["k2"], **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _three_launch(c, gpu, prec):
    from diarizen_amd import ops
    C, H, W, Cp, Wp = c["C"], c["H"], c["W"], c["Cp"], c["Wp"]
    prev, mid = c["prev"].to(gpu), c["mid"].to(gpu)
    scb, out = torch.zeros_like(mid), torch.zeros_like(mid)
    img, pimg = mid[0].numel(), prev[0].numel()
    interior = ((W + 2) + 1) * C
    centre = ((Wp + 2) + 1) * Cp
    t1, t2 = c["tab1"].to(gpu), c["tab2"].to(gpu)
    am = (lambda x: dict(a_amax=_amax(x))) if prec != 0 else (lambda x: {})
    ops.gemm(prev.reshape(-1)[centre:], c["Ws"].to(gpu), M=H * W, N=C, K=Cp, lda=0, a_rowoff=t2, c_rowoff=t1,
             bias=c["bs"].to(gpu), nz=B, zs=dict(a_z0=pimg, c_z0=img), C_out=scb.reshape(-1)[interior:], precision=prec,
             amax_unit=0, **am(prev))
    ops.gemm(mid.reshape(-1), c["W2"].to(gpu), M=H * W, N=C, K=c["K1"], lda=0, a_rowoff=t1, c_rowoff=t1, kc=3 * C,
             ldk=(W + 2) * C, bias=c["b2"].to(gpu), R=scb.reshape(-1)[interior:], post_relu=True, nz=B,
             zs=dict(a_z0=img, c_z0=img), C_out=out.reshape(-1)[interior:], precision=prec, amax_unit=0, **am(mid))
    torch.cuda.synchronize()
    return out.cpu()


def _check(c, gpu, mode, label):
    prec = MODES[mode]
    out = _fused(c, gpu, prec)
    assert torch.count_nonzero(out[:, 0]) == 0 and torch.count_nonzero(out[:, :, 0]) == 0 and \
        torch.count_nonzero(out[:, -1]) == 0 and torch.count_nonzero(out[:, :, -1]) == 0, "border written"
    got = out[:, 1:-1, 1:-1]
    e_ref = _rel(got, c["ref"])
    e_3 = _rel(got, _three_launch(c, gpu, prec)[:, 1:-1, 1:-1])
    print(f"[{label} {mode}] vs float64 {e_ref:.2e} of |max|; vs three launches {e_3:.2e} of |max|")
    assert e_ref <= 1e-5
    assert e_3 <= 2e-6


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_second_segment_matches_float64_and_three_launches(built_lib, gpu, geom, mode):
    _check(_case(geom), gpu, mode, geom)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", ["second_source_2^10_larger", "first_source_2^10_larger"])
def test_one_scale_for_two_sources_of_unequal_magnitude(built_lib, gpu, which, mode):
    """the fp16 forms scale BOTH segments by the power of two of max(a_amax, a2_amax): a source 2^10 below the other keeps its
    two terms — same bars"""
    gains = dict(prev_gain=1024.0) if which.startswith("second") else dict(mid_gain=1024.0)
    _check(_case("c32_3x5", **gains), gpu, mode, which)


@pytest.mark.parametrize("mode", list(MODES))
def test_columns_beyond_k2_are_never_read(built_lib, gpu, mode):
    """k2 = 32 leaves half of the last 64-column tile to zero weights; the 32 floats behind a centre pixel's channels are its
    right-hand neighbour (odd x: no stride-2 patch centre).  Non-finite values there — a stale slot of a skipped window — must
    not reach the sum: 0 x NaN is NaN, so the kernel must not multiply them at all."""
    c = _case("c32_3x5")
    clean = _fused(c, gpu, MODES[mode])
    dirty = c["prev"].clone()
    dirty[:, 1:-1, 2:-1:2] = float("nan")      # padded x = 2, 4, ... = image x = 1, 3, ...
    dirty[0, 1, 2, :4] = float("inf")
    dirty[1, 3, 4, 7] = -float("inf")
    out = _fused(c, gpu, MODES[mode], prev=dirty, prev_amax=_amax(c["prev"].to(gpu)))
    assert torch.isfinite(out).all()
    assert torch.equal(out, clean)


@pytest.mark.parametrize("mode", list(MODES))
def test_first_segment_must_end_on_a_k_tile(built_lib, gpu, mode):
    """K1 % 64 != 0 -> DZN_E_INVALID"""
    from diarizen_amd._lib import DznError
    c = _case("c32_3x5")
    with pytest.raises(DznError, match="invalid argument"):
        _fused(c, gpu, MODES[mode], k1=c["K1"] - 32)


def test_mx_and_presplit_forms_refuse_a_second_segment(built_lib, gpu):
    from diarizen_amd import ops
    from diarizen_amd._lib import DznError
    c = _case("c32_3x5")
    with pytest.raises(DznError, match="invalid argument"):
        _fused(c, gpu, 4, precision_kw=dict(mx=True))
    K = c["Wcat"].shape[1]
    A = torch.randn(128, K, generator=torch.Generator().manual_seed(1)).to(gpu)
    with pytest.raises(DznError, match="invalid argument"):
        ops.gemm(A, c["Wcat"].to(gpu), precision=2, a_planes=ops.split_rows(A), A2=c["prev"].to(gpu).reshape(-1),
                 a2_rowoff=torch.zeros(128, dtype=torch.int32, device=gpu), k1=c["K1"], k2=c["k2"])


def test_engine_fused_and_three_launch_forms_agree(built_lib, gpu, tmp_path):
    """dzn_embed_forward, 3 windows of 2 s, seeded ResNet weights, the middle window silent: one engine per form, each in a
    fresh process (the switch is read at dzn_create).  cosine >= 0.9999, max |d| <= 1e-5 of |max|; the silent window is the
    pooled bias bit for bit in both; a HIP-graph replay reproduces the eager bits; the fused engine launches the K = 640 / 1216 /
    2432 contractions and no shortcut launch."""
    from testkit.weights import emb_state_dict
    worker = os.path.join(os.path.dirname(__file__), "_shortcut_worker.py")
    procs = {}
    for form in ("fused", "three"):
        env = dict(os.environ)
        env.pop("DZN_NO_SHORTCUT_FUSION", None)
        if form == "three":
            env["DZN_NO_SHORTCUT_FUSION"] = "1"
        procs[form] = subprocess.Popen([sys.executable, worker, str(tmp_path / f"{form}.pt")], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for form, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0 and "SHORTCUT_WORKER_OK" in log, f"{form}: exit {p.returncode}\n{log[-3000:]}"
        res[form] = torch.load(tmp_path / f"{form}.pt")
    a, b = res["fused"]["emb"], res["three"]["emb"]
    cos = torch.nn.functional.cosine_similarity(a.reshape(-1, 256).double(), b.reshape(-1, 256).double(), dim=-1).min().item()
    d = (a.double() - b.double()).abs().max().item() / b.double().abs().max().item()
    print(f"[engine] fused vs three launches: min cos {cos:.8f}, max |d| {d:.2e} of |max|")
    assert cos >= 0.9999 and d <= 1e-5
    bias = emb_state_dict(0)["resnet.seg_1.bias"]
    for form in res:
        assert all(torch.equal(res[form]["emb"][1, s], bias) for s in range(4)), f"{form}: silent window is not the bias"
        assert not torch.equal(res[form]["emb"][0, 0], bias)
        assert res[form]["replay_equal"], f"{form}: graph replay differs from the eager call"
    shapes = {form: [n for n in res[form]["kernels"] if n.startswith("gemm_")] for form in res}
    for n, k in ((64, 640), (128, 1216), (256, 2432)):
        assert any(f" N{n} K{k} " in s for s in shapes["fused"]), (n, k, shapes["fused"])
    for n, k in ((64, 32), (128, 64), (256, 128)):
        assert not any(f" N{n} K{k} " in s for s in shapes["fused"]), (n, k, shapes["fused"])
        assert any(f" N{n} K{k} " in s for s in shapes["three"]), (n, k, shapes["three"])
