"""The front-end matrix (device): conv0_kernel, split_weights_h2_frag_kernel and conv01_ws_kernel through their dzn_op_* entry
points against the float64 references and derived bounds of tests/_frontend_cases.py, at the shapes where these kernels handle
an edge by hand (the 64-frame block and the wavefront stride of conv0; the 127-row tile, its seams, both parities of T0 and the
persistent (window, tile) loop of the fused kernel).  Every buffer lies between pattern bands and is compared bit for bit outside
what the kernel owns, every launch runs twice (the same bits) and once more with the OTHER windows' waveforms changed (window 0's
bits stay).  Each test prints its worst error / bound ratio.  test_frontend_kernels_host.py shows what the bounds let through
and what they do not."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _frontend_cases as fc
from _frontend_cases import F32, F64, worst_ratio
from diarizen_amd import ops
from diarizen_amd._lib import DznError
from test_small_kernels_gpu import Buf, Worst as _Worst, _dev, _finish

pytestmark = pytest.mark.gpu


class Worst(_Worst):
    def done(self):
        print(f"\n[front-end matrix] {self.name}: worst error / bound = {self.r:.3f} at {self.at}")
        assert self.r < 1.0, f"{self.name}: error / bound = {self.r:.3f} at {self.at}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _other_windows(inp):
    """the same inputs with every waveform after window 0 changed (and its statistics with it)"""
    alt = dict(inp)
    wave = inp["wave"].copy()
    wave[1:] = -3.0 * wave[1:] + 0.01
    alt["wave"] = wave
    if inp["stats"] is not None:
        alt["stats"] = fc._wave_stats(wave)
        assert np.array_equal(alt["stats"][0], inp["stats"][0])
    return alt


# ---- conv0 ----------------------------------------------------------------------------------------------------------------
def _c0(dev, c, inp, lnq):
    B, N, C0, Cp, T0 = c["B"], c["N"], c["C0"], c["Cp"], c["T0"]
    wb = Buf(dev, B, N, inp["wave"]).arm()
    ob = Buf(dev, B * T0, Cp).arm(True)
    ln = c["mode"] != "raw"
    ops.conv0(wb.v, _dev(inp["w"], dev), ob.v, B=B, N=N, C0=C0, Cp=Cp, k=c["k"], s=c["s"], T0=T0, layer_norm=int(ln),
              stats=_dev(inp["stats"], dev), gamma=_dev(inp["gamma"], dev) if ln else None, beta=_dev(inp["beta"], dev) if ln else None,
              lnq=_dev(lnq, dev) if c["mode"] == "lnq" else None, eps=fc.EPS_LN)
    _finish([wb, ob], f"conv0 {c}")
    return ob.get().reshape(B, T0, Cp)


def _c0_lnq(c, inp):
    return ops.conv0_lnq(inp["w"], c["C0"], c["k"])


def test_conv0(built_lib, gpu):
    worst = {m: Worst(f"conv0 [{m}]") for m in fc.MODES}
    for c in fc.c0_cases():
        inp = fc.c0_inputs(c)
        lnq = _c0_lnq(c, inp)
        got = _c0(gpu, c, inp, lnq)
        assert np.isfinite(got).all(), f"a stored element is not finite: {c}"
        assert not got[..., c["C0"]:].any(), f"columns [C0, Cp) are not zero: {c}"
        worst[c["mode"]].add(got, fc.c0_run(c, inp)["out"], fc.c0_bound(c, inp)["out"], c)
        assert np.array_equal(_bits(got), _bits(_c0(gpu, c, inp, lnq))), f"a second launch gives other bits: {c}"
        alt = _c0(gpu, c, _other_windows(inp), lnq)
        assert np.array_equal(_bits(alt[0]), _bits(got[0])), f"window 0 follows its neighbours: {c}"
    for w in worst.values():
        w.done()


def test_conv0_stress_case_holds_on_both_statistics_paths(built_lib, gpu):
    """DC-blocking taps on a slow sine with a DC offset: the samples of a frame lie almost along the null directions of the taps'
    covariance.  Both the factor form (lnq) and the sums over the computed outputs hold the float64 two-pass reference; the plain
    product form x^T Q x would not (host test: error / bound 3.5).  Measured on an MI355X: error / bound 0.394 (lnq), 0.270 (wave sums)."""
    for mode in ("lnq", "wave"):
        c = next(c for c in fc.c0_cases() if c["stress"] and c["mode"] == mode)
        inp = fc.c0_inputs(c)
        got = _c0(gpu, c, inp, _c0_lnq(c, inp))
        r = worst_ratio(got, fc.c0_run(c, inp)["out"], fc.c0_bound(c, inp)["out"])
        print(f"\n[front-end matrix] conv0 stress case [{mode}]: error / bound = {r:.3f}")
        assert r < 1.0, f"conv0 stress case [{mode}]: error / bound = {r:.3f}"


def test_conv0_refusals(built_lib, gpu):
    big, out = torch.zeros(1 << 20, device=gpu), torch.zeros(1 << 20, device=gpu)
    ok = dict(B=1, N=100, C0=8, Cp=8, k=10, s=5, T0=19, layer_norm=1, gamma=big, beta=big)
    ops.conv0(big, big, out, **ok)                           # the base geometry is served
    torch.cuda.synchronize()
    bad = [("null wave", dict(wave=None)), ("null w", dict(w=None)), ("null out", dict(out=None)), ("Cp < C0", dict(Cp=4)),
           ("Cp % 4", dict(C0=6, Cp=6)), ("k < 1", dict(k=0)), ("s < 1", dict(s=0)), ("reads past the window", dict(T0=20)),
           ("layer_norm without gamma", dict(gamma=None)), ("layer_norm without beta", dict(beta=None)), ("layer_norm = 2", dict(layer_norm=2)),
           ("k > 10", dict(k=11, N=200)), ("C0 > 512", dict(C0=516, Cp=516)), ("s > 8", dict(s=9, N=400))]
    for what, ch in bad:
        kw = dict(ok, **{k: v for k, v in ch.items() if k not in ("wave", "w", "out")})
        args = [None if n in ch else t for n, t in (("wave", big), ("w", big), ("out", out))]
        with pytest.raises(DznError):
            ops.conv0(*args, **kw)
            pytest.fail(f"conv0 served: {what}")
    torch.cuda.synchronize()


# ---- split_weights_h2_frag ------------------------------------------------------------------------------------------------
def test_split_weights_h2_frag_is_split_weights_h2_reindexed(built_lib, gpu):
    for rows, K in fc.FRAG_SHAPES:
        W = fc.frag_inputs(rows, K)
        Wd = _dev(W, gpu)
        planes, cs = ops.split_weights_h2(Wd)
        wb = Buf(gpu, rows, K, W).arm()
        pb = Buf(gpu, 1, rows * K, dtype=torch.int32).arm(True)          # rows K 2 fp16 = rows K 4 bytes
        sb = Buf(gpu, 1, rows).arm(True)
        ops.split_weights_h2_frag(wb.t, out=pb.v, col_scale=sb.v)
        _finish([wb, pb, sb], f"split_weights_h2_frag {rows} x {K}")
        got = pb.v.view(torch.int16).cpu().numpy().view(np.uint16).reshape(K // 32, rows // 16, 2, 16, 32)
        want = fc.frag_reindex(fc.h2_natural(planes.cpu().numpy().view(np.uint16)))
        assert np.array_equal(got, want), f"fragment-major planes differ from split_weights_h2: {rows} x {K}"
        assert np.array_equal(_bits(sb.get()[0]), _bits(cs.cpu().numpy())), f"col_scale differs: {rows} x {K}"
        ref_planes, ref_inv = fc.h2_split(W)                # and both are the stated split
        assert np.array_equal(want, fc.frag_reindex(ref_planes)) and np.array_equal(sb.get()[0], ref_inv)
        assert sb.get()[0][rows // 2] == 1.0 and not got[:, (rows // 2) // 16, :, (rows // 2) % 16].any()
    print("\n[front-end matrix] split_weights_h2_frag: exact on every shape")
    Wd = torch.zeros(64, 64, device=gpu)
    o, s = torch.zeros(64 * 64, dtype=torch.int32, device=gpu), torch.zeros(64, device=gpu)
    for what, Wbad in (("rows % 16", Wd[:24]), ("K % 32", Wd[:, :48].contiguous())):
        with pytest.raises(DznError):
            ops.split_weights_h2_frag(Wbad, out=o, col_scale=s)
            pytest.fail(f"split_weights_h2_frag served: {what}")


# ---- conv01 ---------------------------------------------------------------------------------------------------------------
HIGH = 1.0e6                    # a tracker preload above every |out|


def _c01(dev, c, inp, prep):
    B, N, C0, C1, T0, T1 = c["B"], c["N"], c["C0"], c["C1"], c["T0"], c["T1"]
    wb = Buf(dev, B, N, inp["wave"]).arm()
    ob = Buf(dev, B * T1, fc.N1P).arm(True)
    am = None
    if c["amax"] != "none":
        am = Buf(dev, 1, B, np.full((1, B), HIGH if c["amax"] == "high" else 0.0, F32)).arm(True if c["ln"] else None)
    ops.conv01_fused(wb.v, prep["w0"], prep["gamma0"], prep["beta0"], prep["lnq"], prep["W2h"], prep["cs"], ob.v, B=B, N=N, C0=C0, T0=T0,
                     T1=T1, act_bound=inp["act_bound"], wstats=_dev(inp["stats"], dev), gamma1=prep["gamma1"] if c["ln"] else None,
                     beta1=prep["beta1"] if c["ln"] else None, C1=C1, amax1=am and am.v, eps=fc.EPS_LN)
    _finish([b for b in (wb, ob, am) if b is not None], f"conv01_fused {c}")
    out = dict(out=ob.get().reshape(B, T1, fc.N1P))
    if am is not None:
        out["amax"] = am.get()[0]
    return out


def _c01_prep(dev, c, inp):
    W2h, cs = ops.split_weights_h2_frag(_dev(inp["W"], dev))
    p = {k: _dev(inp[k], dev) for k in ("gamma1", "beta1")}
    p.update(w0=_dev(inp["w"], dev), gamma0=_dev(inp["gamma"], dev), beta0=_dev(inp["beta"], dev), W2h=W2h, cs=cs,
             lnq=_dev(ops.conv0_lnq(inp["w"], c["C0"], 10), dev))
    return p


def _c01_case(dev, c, worst, rerun=True):
    inp = fc.c01_inputs(c)
    prep = _c01_prep(dev, c, inp)
    got = _c01(dev, c, inp, prep)
    o = got["out"]
    assert np.isfinite(o).all(), f"a stored element is not finite: {c}"
    assert not o[..., c["C1"]:].any(), f"columns [C1, 160) are not zero: {c}"
    worst["ln" if c["ln"] else "raw"].add(o, fc.c01_run(c, inp)["out"], fc.c01_bound(c, inp)["out"], c)
    if "amax" in got:
        pre = F32(HIGH if c["amax"] == "high" else 0.0)
        want = np.maximum(pre, np.abs(o).reshape(c["B"], -1).max(1)) if c["ln"] else np.full(c["B"], pre, F32)
        assert np.array_equal(_bits(got["amax"]), _bits(want.astype(F32))), f"tracker is not max(preload, max |out|): {c}"
    if rerun:
        again = _c01(dev, c, inp, prep)
        assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got), f"a second launch gives other bits: {c}"
        alt = _c01(dev, c, _other_windows(inp), prep)
        assert np.array_equal(_bits(alt["out"][0]), _bits(o[0])), f"window 0 follows its neighbours: {c}"
    return inp, prep, o


def _P(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def test_conv01(built_lib, gpu):
    worst = dict(raw=Worst("conv01 [raw]"), ln=Worst("conv01 [LayerNorm epilogue]"))
    for c in fc.c01_cases(_P(gpu))[:-3]:
        _c01_case(gpu, c, worst)
    for w in worst.values():
        w.done()


@pytest.mark.parametrize("which", (-3, -2, -1))
def test_conv01_persistent_loop(built_lib, gpu, which):
    """more (window, tile) items than workgroups: workgroup 0 walks three items and the others two (B = 2 P + 1, one tile each),
    and consecutive items of a workgroup belong to different windows (B = P + 1, two tiles each, with and without the epilogue
    LayerNorm); every window has its own waveform, so the statistics or the window index of the item before would show"""
    P = _P(gpu)
    c = fc.c01_cases(P)[which]
    assert c["B"] * -(-c["T1"] // fc.TILE) > P
    worst = dict(raw=Worst("conv01 persistent loop [raw]"), ln=Worst("conv01 persistent loop [LayerNorm epilogue]"))
    _c01_case(gpu, c, worst)
    worst["ln" if c["ln"] else "raw"].done()


def test_conv01_agrees_with_conv0_then_float64_conv1(built_lib, gpu):
    """at no extra bound: the unfused kernel's activations (lnq statistics) through the float64 conv1 (and epilogue) land inside
    the fused kernel's bound of the fused kernel's output"""
    worst = Worst("conv01 against conv0 + float64 conv1")
    cases = fc.c01_cases(_P(gpu))[:-3]
    for c in (cases[4], cases[7], cases[10], cases[11]):
        inp = fc.c01_inputs(c)
        prep = _c01_prep(gpu, c, inp)
        fused = _c01(gpu, c, inp, prep)["out"]
        c0 = dict(c, Cp=c["C0"], mode="lnq")
        a = _c0(gpu, c0, inp, prep["lnq"].cpu().numpy())
        worst.add(fused, fc.c01_run(c, inp, a=a.astype(F64))["out"], fc.c01_bound(c, inp)["out"], c)
    worst.done()


def test_conv01_refusals(built_lib, gpu):
    big, out = torch.zeros(1 << 20, device=gpu), torch.zeros(1 << 20, device=gpu)
    pos = dict(wave=big, w0=big, gamma0=big, beta0=big, lnq=big, W2h=big, col_scale=big, out=out)
    ok = dict(B=1, N=40, C0=128, T0=7, T1=3, act_bound=1.0, N1p=160, gamma1=big, beta1=big, C1=153)
    names = list(pos)

    def call(ch):
        p = dict(pos, **{k: v for k, v in ch.items() if k in pos})
        kw = dict(ok, **{k: v for k, v in ch.items() if k not in pos})
        return ops.conv01_fused(*[p[n] for n in names], **kw)

    call({})                                                # the base geometry is served
    torch.cuda.synchronize()
    bad = [("null wave", dict(wave=None)), ("null w0", dict(w0=None)), ("null gamma0", dict(gamma0=None)), ("null beta0", dict(beta0=None)),
           ("null out", dict(out=None)), ("frame T0 - 1 past the window", dict(N=39)), ("T1 past conv0's frames", dict(T1=4, T0=8, N=45)),
           ("T0 < 3", dict(T0=2, T1=1)),
           # the launcher's own
           ("C0 < 128", dict(C0=64)), ("C0 % 64", dict(C0=160)), ("N1p != 160", dict(N1p=128)), ("C1 <= 80", dict(C1=80)),
           ("C1 > N1p", dict(C1=161)), ("no lnq", dict(lnq=None)), ("no W2h", dict(W2h=None)), ("no col_scale", dict(col_scale=None)),
           ("act_bound <= 0", dict(act_bound=0.0)), ("gamma1 without beta1", dict(beta1=None))]
    for what, ch in bad:
        with pytest.raises(DznError):
            call(ch)
            pytest.fail(f"conv01_fused served: {what}")
    torch.cuda.synchronize()
