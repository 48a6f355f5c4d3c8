"""The image-kernel matrix (device): csrc/conv_split.hip, csrc/resblock_fused.hip and csrc/resblock_ws.hip through the entry points
that launch them as the engine does (dzn_op_*_ex: caller-owned output, |max| trackers, device-chosen image lists, explicit number
of terms) against the float64 reference and the derived per-element bound of tests/_image_cases.py, at the shapes where these
kernels handle an edge by hand.  Every buffer lies between pattern bands (a NaN as fp32) and the output itself starts as the
pattern: an element nobody stored is not finite, an element stored outside the interior of a listed image is a changed bit.  The
trackers are held to max(preload, max |out[b]|) bit for bit.  Each test prints its worst error / bound ratio per kernel form.
test_image_kernels_host.py shows what the bounds let through and what they do not."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _image_cases as ic
from _image_cases import F32, GUARD, PATTERN, worst_ratio
from diarizen_amd import ops
from diarizen_amd._lib import DznError

pytestmark = pytest.mark.gpu


class Band:
    """GUARD | shape | GUARD elements on the device, the pattern everywhere, then `data` in the middle"""

    def __init__(self, dev, shape, data=None, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.raw = torch.full((2 * GUARD + self.n,), PATTERN, dtype=torch.int32, device=dev)
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(*shape)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dev))
        self.before = self.bits()

    def bits(self):
        return self.raw.cpu().numpy().view(np.uint32).copy()

    def unchanged(self, what, owned=None):
        """every element outside `owned` (a mask over shape) holds the bits it held before the launch"""
        now, keep = self.bits(), np.ones(self.raw.numel(), bool)
        if owned is not None:
            keep[GUARD:GUARD + self.n] = ~np.asarray(owned, bool).reshape(-1)
        bad = np.nonzero((now != self.before) & keep)[0]
        assert bad.size == 0, f"{what}: {bad.size} elements outside what the launch owns changed, first at {int(bad[0]) - GUARD}"

    def get(self):
        return self.t.cpu().numpy()


class Worst:
    def __init__(self, name):
        self.name, self.r, self.at = name, 0.0, None

    def add(self, got, ref, bound, case):
        r = worst_ratio(got, ref, bound)
        if r >= self.r:
            self.r, self.at = r, case
        return r

    def done(self):
        print(f"\n[image-kernel matrix] {self.name}: worst error / bound = {self.r:.3f} at {self.at}")
        assert self.r < 1.0, f"{self.name}: error / bound = {self.r:.3f} at {self.at}"


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault is sticky: nothing more may run on this context
        pytest.exit(f"{what}: the device reported {e}; the session ends here", returncode=3)


_WEIGHTS = {}


def _weights(dev, C):
    """the device form of _image_cases.weights(C): bf16 three-term planes of w1 (C = 32), fp16 two-term planes + inverse row scales
    of w1 / w2, the folded shifts"""
    if C not in _WEIGHTS:
        w = ic.weights(C)
        d = {k: torch.from_numpy(w[k]).to(dev) for k in ("w1", "w2", "b1", "b2")}
        _WEIGHTS[C] = dict(b1=d["b1"], b2=d["b2"], h1=ops.split_weights_h2(d["w1"]), h2=ops.split_weights_h2(d["w2"]),
                           W31=ops.split_weights(d["w1"]), W32=ops.split_weights(d["w2"]))
    return _WEIGHTS[C]


def _launch(dev, c, inp, form, preload=None, lists="case"):
    """one launch of `form` ("conv", "fused", "ws") as case c describes it -> (out [B, H + 2, W + 2, C] fp32 as stored, tracker [B]
    or None).  Checks what no launch may touch: inputs, borders, unlisted images, bands.  lists: "case", or (z_count, z_list)."""
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    wt, what = _weights(dev, C), f"{form} {c}"
    shape = (B, H + 2, W + 2, C)
    xb, ob, ab = Band(dev, shape, inp["x"]), Band(dev, shape), Band(dev, (B,), inp["amax_in"])
    rb = Band(dev, shape, inp["R"]) if c.get("R") else None
    tb = None if preload is None else Band(dev, (B,), preload)
    zc, zl = ic.list_buffers(c) if lists == "case" else lists
    zcb = None if zc is None else Band(dev, zc.shape, zc, torch.int32)
    zlb = None if zl is None else Band(dev, zl.shape, zl, torch.int32)
    kw = dict(amax_in=ab.t, amax_out=tb and tb.t, z_count=zcb and zcb.t, z_list=zlb and zlb.t)
    if form == "conv":
        if c["np"] == 2:
            ops.conv3x3_c32_ex(xb.t, wt["b1"], ob.t, h2_weights=wt["h1"], R=rb and rb.t, relu=c["relu"], post_relu=c["post"], **kw)
        else:
            ops.conv3x3_c32_ex(xb.t, wt["b1"], ob.t, W3=wt["W31"], R=rb and rb.t, relu=c["relu"], post_relu=c["post"],
                               **dict(kw, amax_in=None))
    else:
        fn = ops.resblock32_fused_ex if form == "fused" else ops.resblock_ws_ex
        fn(xb.t, wt["h1"], wt["b1"], wt["h2"], wt["b2"], inp["l1max1"], inp["bmax1"], ob.t, np=c["np"], **kw)
    _sync(what)
    if lists == "case":
        sel = ic.case_images(c)
    else:                             # half a list is no list
        sel = [int(b) for b in zl[:int(zc[0])]] if (zc is not None and zl is not None) else list(range(B))
    owned = np.zeros(shape, bool)
    owned[sel, 1:-1, 1:-1, :] = True
    ob.unchanged(what + ": out", owned)
    for b_, name in ((xb, "in"), (rb, "R"), (ab, "amax_in"), (zcb, "z_count"), (zlb, "z_list")):
        if b_ is not None:
            b_.unchanged(f"{what}: {name}")
    if tb is not None:
        own = np.zeros(B, bool)
        own[sel] = True
        tb.unchanged(what + ": amax_out", own)
    return ob.get(), None if tb is None else tb.get()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _judge(dev, c, inp, form, worst, ref, bnd):
    """launch, hold every interior element of every listed image to its bound and the tracker to its rule -> out as stored"""
    sel = ic.case_images(c)
    pre = ic.tracker_preload(c, ref)
    out, trk = _launch(dev, c, inp, form, pre)
    got = out[:, 1:-1, 1:-1, :]
    if sel:
        assert np.isfinite(got[sel]).all(), f"{form} {c}: an interior element of a listed image was never stored"
        r = worst.add(got[sel], ref[sel], bnd[sel], c)
        assert r < 1.0, f"{form}: error / bound = {r:.3f} at {c}"
    if pre is None:
        assert trk is None
    else:
        want = ic.tracker_after(c, pre, got)
        assert np.array_equal(_bits(trk), _bits(want)), f"{form} {c}: amax_out {trk} where max(preload, max |out|) = {want}"
    return out


def _same_as_full(dev, c, inp, form, out):
    """a launch over a list stores, for its images, the bits of a launch over all images"""
    sel = ic.case_images(c)
    if c["zl"] == "none" or not sel:
        return
    full, _ = _launch(dev, dict(c, zl="none"), inp, form)
    assert np.array_equal(_bits(out[sel]), _bits(full[sel])), f"{form} {c}: the listed images differ from a launch over all images"


@pytest.mark.parametrize("nterm", [3, 2])
def test_conv(built_lib, gpu, nterm):
    w = Worst(f"conv3x3_c32_split_kernel<{nterm}>")
    for c in ic.conv_cases():
        if c["np"] != nterm:
            continue
        inp = ic.inputs(c)
        ref, bnd = ic.conv_run(c, inp)["out"], ic.conv_bound(c, inp)["out"]
        out = _judge(gpu, c, inp, "conv", w, ref, bnd)
        _same_as_full(gpu, c, inp, "conv", out)
        if c["B"] == 17:        # ... and the bits of B launches of one image each
            for b in ic.case_images(c):
                one = dict(c, B=1, zl="none")
                sub = dict(inp, x=inp["x"][b:b + 1], R=None if inp["R"] is None else inp["R"][b:b + 1], amax_in=inp["amax_in"][b:b + 1])
                alone, _ = _launch(gpu, one, sub, "conv")
                assert np.array_equal(_bits(out[b]), _bits(alone[0])), f"conv {c}: image {b} differs from a launch of its own"
    w.done()


@pytest.mark.parametrize("nterm", [2, 1])
def test_block32_fused_and_ws(built_lib, gpu, nterm):
    """both 32-plane kernels on every case, and the same bits from both (same planes, same scales, same product order)"""
    wf, ww = Worst(f"resblock32_fused_kernel<{nterm}>"), Worst(f"resblock_ws_kernel<32, {nterm}>")
    for c in ic.block_cases(32):
        if c["np"] != nterm:
            continue
        inp = ic.inputs(c)
        ref, bnd = ic.block_run(c, inp)["out"], ic.block_bound(c, inp)["out"]
        fused = _judge(gpu, c, inp, "fused", wf, ref, bnd)
        ws = _judge(gpu, c, inp, "ws", ww, ref, bnd)
        assert np.array_equal(_bits(fused), _bits(ws)), f"resblock_ws (C = 32) and resblock32_fused differ at {c}"
        _same_as_full(gpu, c, inp, "fused", fused)
        _same_as_full(gpu, c, inp, "ws", ws)
    wf.done()
    ww.done()


@pytest.mark.parametrize("nterm", [2, 1])
def test_block64_ws(built_lib, gpu, nterm):
    w = Worst(f"resblock_ws_kernel<64, {nterm}>")
    for c in ic.block_cases(64):
        if c["np"] != nterm:
            continue
        inp = ic.inputs(c)
        out = _judge(gpu, c, inp, "ws", w, ic.block_run(c, inp)["out"], ic.block_bound(c, inp)["out"])
        _same_as_full(gpu, c, inp, "ws", out)
    w.done()


def test_two_convs_against_the_fused_block(built_lib, gpu):
    """conv -> conv (two-term form, the intermediate scaled from its |max| tracker) and the fused block: both inside their float64
    bounds (the chain's with unit_max = the tracker's value for the intermediate), their difference inside the sum of the two"""
    wt = _weights(gpu, 32)
    wc, wd = Worst("conv -> conv (tracked intermediate)"), Worst("fused block - two convs, over the sum of the bounds")
    for c in ic.block_cases(32):
        if c["np"] != 2 or c["zl"] != "none" or c["B"] > 20:
            continue
        inp = ic.inputs(c)
        x, am = torch.from_numpy(inp["x"]).to(gpu), torch.from_numpy(inp["amax_in"]).to(gpu)
        mid, two, trk = torch.zeros_like(x), torch.zeros_like(x), torch.zeros(c["B"], device=gpu)
        ops.conv3x3_c32_ex(x, wt["b1"], mid, h2_weights=wt["h1"], amax_in=am, relu=True, amax_out=trk)
        ops.conv3x3_c32_ex(mid, wt["b2"], two, h2_weights=wt["h2"], amax_in=trk, R=x, post_relu=True)
        fused, _ = _launch(gpu, c, inp, "fused")
        _sync(f"conv -> conv {c}")
        unit = trk.cpu().numpy()
        assert np.array_equal(_bits(unit), _bits(np.abs(mid.cpu().numpy()).reshape(c["B"], -1).max(1))), f"tracker of the intermediate: {c}"
        ref = ic.block_run(c, inp)["out"]
        b_fused, b_two = ic.block_bound(c, inp)["out"], ic.block_bound(c, inp, unit_mid=unit)["out"]
        got2, gotf = two.cpu().numpy()[:, 1:-1, 1:-1], fused[:, 1:-1, 1:-1]
        assert wc.add(got2, ref, b_two, c) < 1.0 and worst_ratio(gotf, ref, b_fused) < 1.0, c
        assert wd.add(gotf, got2, b_fused + b_two, c) < 1.0, c
    wc.done()
    wd.done()


def test_refusals_and_half_given_lists(built_lib, gpu):
    """C other than 32 / 64 and np other than 1 / 2 are refused; a list without a count and a count without a list are launches
    over all images; the two-term conv needs all three of its operands and no W3"""
    c = next(c for c in ic.block_cases(32) if c["np"] == 2 and c["B"] == 3 and c["zl"] == "subset")
    inp, wt = ic.inputs(c), _weights(gpu, 32)
    x, am = torch.from_numpy(inp["x"]).to(gpu), torch.from_numpy(inp["amax_in"]).to(gpu)
    out = torch.zeros_like(x)
    args = (x, wt["h1"], wt["b1"], wt["h2"], wt["b2"], inp["l1max1"], inp["bmax1"], out)
    for bad in (48, 0, 16, 128):
        with pytest.raises(DznError):
            ops.resblock_ws_ex(*args, amax_in=am, C_planes=bad)
    for bad in (0, 3, -1):
        with pytest.raises(DznError):
            ops.resblock_ws_ex(*args, amax_in=am, np=bad)
        with pytest.raises(DznError):
            ops.resblock32_fused_ex(*args, amax_in=am, np=bad)
    with pytest.raises(DznError):
        ops.conv3x3_c32_ex(x, wt["b1"], out, W3=wt["W31"], h2_weights=wt["h1"])            # two-term weights without amax_in
    with pytest.raises(DznError):
        ops.conv3x3_c32_ex(x, wt["b1"], out, W3=wt["W31"], amax_in=am)                     # amax_in without two-term weights
    with pytest.raises(DznError):
        ops.conv3x3_c32_ex(x, wt["b1"], out)                                               # no weights at all
    _sync("refusals")
    assert not out.any(), "a refused launch stored something"
    zc, zl = ic.list_buffers(c)
    cc = dict(c, relu=True, R=False, post=False)
    for form, case in (("fused", c), ("ws", c), ("conv", cc), ("conv", dict(cc, np=3))):
        full, _ = _launch(gpu, dict(case, zl="none"), inp, form)
        for half in ((None, zl), (np.zeros(1, np.int32), None)):
            got, _ = _launch(gpu, case, inp, form, lists=half)
            assert np.array_equal(_bits(got), _bits(full)), f"{form}: {'a list without a count' if half[0] is None else 'a count without a list'} is not a launch over all images"
