"""The small-kernel matrix (device): every launcher of csrc/conformer.hip, frontend.hip, norm.hip and embed.hip through its
dzn_op_* entry point against the float64 reference and the derived bound of tests/_small_cases.py, at the shapes where these
kernels handle an edge by hand.  Every buffer a kernel may write lies between pattern bands (a NaN as fp32) and is compared
bit for bit outside what the kernel owns; every launch runs twice (the same bits) and, where a launch holds several windows,
once more with the OTHER windows' inputs changed (window 0's bits stay).  Each test prints its worst error / bound ratio.
test_small_kernels_host.py shows what the bounds let through and what they do not."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _small_cases as sc
from _small_cases import F32, GUARD, PATTERN, worst_ratio
from diarizen_amd import ops
from diarizen_amd._lib import DznError

pytestmark = pytest.mark.gpu

_FILL = {torch.float32: PATTERN, torch.int32: PATTERN, torch.int64: PATTERN, torch.uint8: 0xA5}


class Buf:
    """GUARD | rows x ld | GUARD elements on the device, pattern-filled; `data` [rows, <= ld] goes into the leading columns.
    off: elements the region is shifted by (1 = a 4-byte-offset view).  arm(mask) remembers the bits, check() holds every
    element outside mask [rows, ld] against them."""

    def __init__(self, dev, rows, ld, data=None, dtype=torch.float32, off=0):
        self.rows, self.ld, self.n = rows, ld, rows * ld
        raw = torch.full((off + 2 * GUARD + self.n,), _FILL[dtype], dtype=torch.int32 if dtype == torch.float32 else dtype, device=dev)
        self.full = raw.view(dtype)
        self.v = self.full[off + GUARD:off + GUARD + self.n]
        self.t = self.v.view(rows, ld)
        self.lo = off + GUARD
        if data is not None:
            d = torch.from_numpy(np.ascontiguousarray(data))
            self.t[:, :d.shape[1]] = d.to(dev)
        self.before = None

    def _bits(self):
        f = self.full
        return (f.view(torch.int32) if f.dtype == torch.float32 else f).cpu().numpy().copy()

    def arm(self, mask=None):
        self.before, self.mask = self._bits(), mask
        return self

    def check(self, what):
        now = self._bits()
        keep = np.ones(now.shape, bool)
        if self.mask is not None:
            keep[self.lo:self.lo + self.n] = ~np.broadcast_to(self.mask, (self.rows, self.ld)).reshape(-1)
        bad = np.nonzero((now != self.before) & keep)[0]
        assert bad.size == 0, f"{what}: {bad.size} elements outside what the kernel owns changed, first at {int(bad[0]) - self.lo}"

    def get(self, cols=None):
        return self.t[:, :cols].cpu().numpy() if cols else self.t.cpu().numpy()


def _cols(rows, ld, n):
    m = np.zeros((rows, ld), bool)
    m[:, :n] = True
    return m


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _finish(bufs, what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault is sticky: nothing more may run on this context
        pytest.exit(f"{what}: the device reported {e}; the session ends here", returncode=3)
    for b in bufs:
        b.check(what)


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs in a second run"


def _others(x, axis0_window0_rows):
    """the same input with everything after window 0 changed"""
    y = x.copy()
    y[axis0_window0_rows:] = -3.0 * y[axis0_window0_rows:] + 1.0
    return y


class Worst:
    def __init__(self, name):
        self.name, self.r, self.at = name, 0.0, None

    def add(self, got, ref, bound, case):
        r = worst_ratio(got, ref, bound)
        if r >= self.r:
            self.r, self.at = r, case
        return r

    def done(self):
        print(f"\n[small-kernel matrix] {self.name}: worst error / bound = {self.r:.3f} at {self.at}")
        assert self.r < 1.0, f"{self.name}: error / bound = {self.r:.3f} at {self.at}"


# ---- glu_dwconv -----------------------------------------------------------------------------------------------------------
def _dw(dev, c, inp, u=None):
    B, L, A = c["B"], c["L"], c["A"]
    ub = Buf(dev, B * L, c["ldu"], (inp["u"] if u is None else u).reshape(B * L, 2 * A)).arm()
    ob = Buf(dev, B * L, c["ldo"]).arm(_cols(B * L, c["ldo"], A))
    ops.glu_dwconv(ub.v, _dev(inp["w"], dev), _dev(inp["bias"], dev), ob.v, B=B, L=L, A=A, ks=c["ks"], ldu=c["ldu"], ldo=c["ldo"])
    _finish([ub, ob], f"glu_dwconv {c}")
    return dict(out=ob.get(A).reshape(B, L, A))


def test_glu_dwconv(built_lib, gpu):
    w = Worst("glu_dwconv")
    for c in sc.dw_cases():
        inp = sc.dw_inputs(c)
        got = _dw(gpu, c, inp)
        w.add(got["out"], sc.dw_run(c, inp)["out"], sc.dw_bound(c, inp)["out"], c)
        _same(got, _dw(gpu, c, inp), c)
        alt = _dw(gpu, c, inp, _others(inp["u"], 1))
        assert np.array_equal(alt["out"][0].view(np.uint32), got["out"][0].view(np.uint32)), f"window 0 follows its neighbours: {c}"
    w.done()


# ---- classify -------------------------------------------------------------------------------------------------------------
def _cls(dev, c, inp):
    rows, A, NC, S = c["rows"], c["A"], c["NC"], c["S"]
    zb = Buf(dev, rows, c["ldz"], inp["z"]).arm()
    lp = None if c["null"] == "logp" else Buf(dev, rows, NC).arm(True)
    ml = None if c["null"] == "multilabel" else Buf(dev, rows, S, dtype=torch.uint8).arm(True)
    so = None if c["null"] == "soft" else Buf(dev, rows, S).arm(True)
    ops.classify(zb.v, _dev(inp["W"], dev), _dev(inp["bias"], dev), _dev(inp["mapping"], dev), rows=rows, A=A, NC=NC, S=S, ldz=c["ldz"],
                 logp=lp and lp.v, multilabel=ml and ml.v, soft=so and so.v)
    _finish([b for b in (zb, lp, ml, so) if b is not None], f"classify {c}")
    return {k: b.get() for k, b in (("logp", lp), ("multilabel", ml), ("soft", so)) if b is not None}


def test_classify(built_lib, gpu):
    wl, wsf = Worst("classify logp"), Worst("classify soft")
    left_out = 0
    for c in sc.cls_cases():
        inp = sc.cls_inputs(c)
        ref, bnd = sc.cls_run(c, inp), sc.cls_bound(c, inp)
        got = _cls(gpu, c, inp)
        _same(got, _cls(gpu, c, inp), c)
        if "logp" in got:
            wl.add(got["logp"], ref["logp"], bnd["logp"], c)
        if "soft" in got:
            wsf.add(got["soft"], ref["soft"], bnd["soft"], c)
        if "multilabel" in got:
            keep = ~bnd["unresolved"]
            left_out += int((~keep).sum())
            assert np.array_equal(got["multilabel"][keep], ref["multilabel"][keep]), f"multilabel (the first maximum wins): {c}"
    print(f"\n[small-kernel matrix] classify: {left_out} rows left out of the multilabel equality")
    wl.done()
    wsf.done()


# ---- groupnorm_gelu -------------------------------------------------------------------------------------------------------
def _gn(dev, c, inp, x=None):
    B, T, C, Cp, ld = c["B"], c["T"], c["C"], c["Cp"], c["ld"]
    xb = Buf(dev, B * T, ld, (inp["x"] if x is None else x).reshape(B * T, Cp))
    yb = xb if c["inplace"] else Buf(dev, B * T, ld)
    xb.arm(_cols(B * T, ld, Cp) if c["inplace"] else None)
    yb.arm(_cols(B * T, ld, Cp))
    nst = ops.gn_stats_floats(B, T, C, Cp)
    assert nst == 2 * B * C + 2 * B * ((T + 127) // 128) * Cp
    st = Buf(dev, 1, nst).arm(True)
    am = Buf(dev, 1, B, np.zeros((1, B), F32)).arm(True) if c["amax"] else None
    ops.groupnorm_gelu(xb.v, yb.v, _dev(inp["gamma"], dev), _dev(inp["beta"], dev), st.v, B=B, T=T, C=C, Cp=Cp, ld=ld, eps=sc.EPS_LN,
                       amax=am and am.v)
    _finish([b for b in (xb, yb, st, am) if b is not None], f"groupnorm_gelu {c}")
    out = dict(y=yb.get(Cp).reshape(B, T, Cp))
    if am is not None:
        out["amax"] = am.get()[0]
    return out


def test_groupnorm_gelu(built_lib, gpu):
    w = Worst("groupnorm_gelu")
    for c in sc.gn_cases():
        inp = sc.gn_inputs(c)
        got = _gn(gpu, c, inp)
        w.add(got["y"], sc.gn_run(c, inp)["y"], sc.gn_bound(c, inp)["y"], c)
        assert not got["y"][..., c["C"]:].any(), f"columns [C, Cp) are not zero: {c}"
        if c["amax"]:
            assert np.array_equal(got["amax"], np.abs(got["y"]).reshape(c["B"], -1).max(1)), f"tracker is not max |y|: {c}"
        _same(got, _gn(gpu, c, inp), c)
        alt = _gn(gpu, c, inp, _others(inp["x"], 1))
        assert np.array_equal(alt["y"][0].view(np.uint32), got["y"][0].view(np.uint32)), f"window 0 follows its neighbour: {c}"
    w.done()


def test_groupnorm_gelu_chunk_merge_against_one_chunk(built_lib, gpu):
    """T = 129: the last chunk holds ONE row.  The statistics of the float64 reference over all rows are what the merge of a
    128-row and a 1-row chunk must give; a chunk weighted as 128 rows moves y by about one part in 129 (host test)."""
    c = next(c for c in sc.gn_cases() if c["T"] == 129 and c["C"] == 153)
    inp = sc.gn_inputs(c)
    inp["x"][:, 128, 2:c["C"]] += 40.0                     # the lonely row far from the first chunk's mean
    got = _gn(gpu, c, inp)
    assert worst_ratio(got["y"], sc.gn_run(c, inp)["y"], sc.gn_bound(c, inp)["y"]) < 1.0


# ---- layernorm_t ----------------------------------------------------------------------------------------------------------
def _ln(dev, c, inp):
    rows, C, Cpad = c["rows"], c["C"], c["Cpad"]
    need = max(C, Cpad)
    ld, off = need + c["pad"], 1 if c["path"] == "offset" else 0
    xb = Buf(dev, rows, ld, inp["x"], off=off)
    yb = xb if c["inplace"] else Buf(dev, rows, ld, off=off)
    xb.arm(_cols(rows, ld, need) if c["inplace"] else None)
    yb.arm(_cols(rows, ld, need))
    unit = c["amax_unit"]
    am = None
    if unit is not None:
        units = 1 if unit == 0 else -(-rows // unit)
        am = Buf(dev, 1, units, np.zeros((1, units), F32)).arm(True)
    ops.layernorm_t(xb.v, _dev(inp["gamma"], dev), _dev(inp["beta"], dev), rows=rows, C=C, Cpad=Cpad, ldx=ld, out=yb.v, ldy=ld,
                    post=_dev(inp["post"], dev), eps=sc.EPS_LN, gelu=c["gelu"], amax=am and am.v, amax_unit=unit or 0)
    _finish([b for b in (xb, yb, am) if b is not None], f"layernorm {c}")
    out = dict(y=yb.get(need))
    if am is not None:
        out["amax"] = am.get()[0]
    return out


def test_layernorm_t(built_lib, gpu):
    worst = {p: Worst(f"layernorm ({p})") for p in ("v4", "offset", "wide")}
    for c in sc.ln_cases():
        inp = sc.ln_inputs(c)
        got = _ln(gpu, c, inp)
        C = c["C"]
        worst[c["path"]].add(got["y"][:, :C], sc.ln_run(c, inp)["y"], sc.ln_bound(c, inp)["y"], c)
        assert not got["y"][:, C:].any(), f"columns [C, Cpad) are not zero: {c}"
        if c["amax_unit"] is not None:
            unit = c["amax_unit"] or c["rows"]
            want = np.array([np.abs(got["y"][r:r + unit, :C]).max() for r in range(0, c["rows"], unit)], F32)
            assert np.array_equal(got["amax"], want), f"tracker is not max |y| of its unit: {c}"
        _same(got, _ln(gpu, c, inp), c)
    for w in worst.values():
        w.done()


def test_layernorm_entry_points_agree(built_lib, gpu):
    """dzn_op_layernorm is dzn_op_layernorm_t without post and tracker: the same bits"""
    g = np.random.default_rng(3)
    x = _dev(g.standard_normal((77, 160)).astype(F32), gpu)
    gam, bet = _dev(g.standard_normal(153).astype(F32), gpu), _dev(g.standard_normal(153).astype(F32), gpu)
    a = ops.layernorm(x, gam, bet, C_true=153, gelu=True)
    b = torch.empty_like(x)
    ops.layernorm_t(x, gam, bet, rows=77, C=153, Cpad=160, ldx=160, out=b, ldy=160, eps=1e-5, gelu=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- wave_stats -----------------------------------------------------------------------------------------------------------
def _wv(dev, N, inp, w=None):
    wb = Buf(dev, 3, N, inp["w"] if w is None else w).arm()
    sb = Buf(dev, 3, 2).arm(True)
    ops.wave_stats(wb.v, 3, N, sc.EPS_LN, out=sb.v)
    _finish([wb, sb], f"wave_stats {N}")
    return dict(stats=sb.get())


def test_wave_stats(built_lib, gpu):
    w = Worst("wave_stats")
    for N in sc.WS_N:
        inp = sc.wv_inputs(N)
        got = _wv(gpu, N, inp)
        w.add(got["stats"], sc.wv_run(N, inp)["stats"], sc.wv_bound(N, inp)["stats"], N)
        _same(got, _wv(gpu, N, inp), N)
        alt = _wv(gpu, N, inp, _others(inp["w"], 1))
        assert np.array_equal(alt["stats"][0].view(np.uint32), got["stats"][0].view(np.uint32))
    w.done()


# ---- pad_rows, col_scale, ws_accum, ws_sum --------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 64])
def test_pad_rows_exact(built_lib, gpu, pad):
    g = np.random.default_rng(11)
    for L, D in ((1, 4), (5, 768), (399, 12)):
        B, Lp = 2, L + 2 * pad + 1
        x = g.standard_normal((B, L, D)).astype(F32)
        xb = Buf(gpu, B * L, D, x.reshape(B * L, D)).arm()
        pb = Buf(gpu, B * Lp, D).arm(True)
        ops.pad_rows(xb.v, pb.v, B=B, L=L, Lp=Lp, pad=pad, D=D)
        _finish([xb, pb], f"pad_rows {L} {D} {pad}")
        want = np.zeros((B, Lp, D), F32)
        want[:, pad:pad + L] = x
        assert np.array_equal(pb.get().reshape(B, Lp, D).view(np.uint32), want.view(np.uint32))


def test_col_scale_exact_and_leaves_the_pad_columns(built_lib, gpu):
    g = np.random.default_rng(12)
    for rows, C, ld in ((1, 1, 4), (37, 30, 40), (1027, 512, 520)):
        x, s = g.standard_normal((rows, C)).astype(F32), g.standard_normal(C).astype(F32)
        xb = Buf(gpu, rows, ld, x).arm(_cols(rows, ld, C))
        ops.col_scale(xb.v, _dev(s, gpu), rows=rows, C_true=C, ld=ld)
        _finish([xb], f"col_scale {rows} {C} {ld}")
        assert np.array_equal(xb.get(C).view(np.uint32), (x * s).view(np.uint32))


@pytest.mark.parametrize("n", sc.WSUM_SIZES)
def test_ws_sum_is_the_ws_accum_chain(built_lib, gpu, n):
    g = np.random.default_rng(n)
    xs = [g.standard_normal(n).astype(F32) for _ in range(max(sc.WSUM_COUNTS))]
    dx = [_dev(x, gpu) for x in xs]
    w = Worst(f"ws_sum / ws_accum (n = {n})")
    for k in sc.WSUM_COUNTS:
        ws = sc.wsum_weights(k)
        a, b = Buf(gpu, 1, n).arm(True), Buf(gpu, 1, n).arm(True)
        ops.ws_sum(dx[:k], ws, a.v, n)
        for j in range(k):
            ops.ws_accum(dx[j], b.v, ws[j], j == 0, n)
        _finish([a, b], f"ws_sum {n} {k}")
        ga, gb = a.get()[0], b.get()[0]
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), f"ws_sum is not the ws_accum chain: n = {n}, k = {k}"
        assert np.array_equal(ga.view(np.uint32), sc.wsum_run(xs[:k], ws, F32).view(np.uint32)), "not product-then-add in list order"
        w.add(ga, sc.wsum_run(xs[:k], ws), sc.wsum_bound(xs[:k], ws), k)
    w.done()


# ---- frame_prep -----------------------------------------------------------------------------------------------------------
def _fp(dev, c, inp, wave=None):
    B, T, Kp = c["B"], c["T"], c["Kp"]
    wv = inp["wave"] if wave is None else wave
    wb = Buf(dev, 1, wv.size, wv[None]).arm()
    fb = Buf(dev, B * T, Kp).arm(True)
    ops.frame_prep(wb.v, _dev(inp["window"], dev), fb.v, B=B, stride=c["stride"], T=T, flen=c["flen"], fshift=c["fshift"], Kp=Kp,
                   preemph=sc.PREEMPH)
    _finish([wb, fb], f"frame_prep {c}")
    return dict(frames=fb.get())


def test_frame_prep(built_lib, gpu):
    w = Worst("frame_prep")
    for c in sc.fp_cases():
        inp = sc.fp_inputs(c)
        got = _fp(gpu, c, inp)
        w.add(got["frames"], sc.fp_run(c, inp)["frames"], sc.fp_bound(c, inp)["frames"], c)
        assert not got["frames"][:, c["flen"]:].any(), f"columns [flen, Kp) are not zero: {c}"
        _same(got, _fp(gpu, c, inp), c)
        if c["stride"] >= c["span"]:
            alt = _fp(gpu, c, inp, _others(inp["wave"], c["span"]))
            T = c["T"]
            assert np.array_equal(alt["frames"][:T].view(np.uint32), got["frames"][:T].view(np.uint32)), f"signal 0 follows signal 1: {c}"
    w.done()


# ---- power, log_cmn, log_cmn_gather ---------------------------------------------------------------------------------------
def test_power(built_lib, gpu):
    w = Worst("power")
    for c in sc.mel_cases():
        inp = sc.pw_inputs(c)
        sb = Buf(gpu, c["T"], 2 * c["NB"], inp["spec"]).arm()
        pb = Buf(gpu, c["T"], c["NB"]).arm(True)
        ops.power(sb.v, pb.v, rows=c["T"], nb=c["NB"])
        _finish([sb, pb], f"power {c}")
        w.add(pb.get(), sc.pw_run(c, inp)["pw"], sc.pw_bound(c, inp)["pw"], c)
    w.done()


def _cmn(dev, c, mel):
    B, T, NB = mel.shape
    mb = Buf(dev, B * T, NB, mel.reshape(B * T, NB)).arm(True)
    ops.log_cmn(mb.v, B=B, T=T, NB=NB, eps=sc.MEL_EPS)
    _finish([mb], f"log_cmn {c}")
    return dict(mel=mb.get().reshape(B, T, NB))


def test_log_cmn(built_lib, gpu):
    w = Worst("log_cmn")
    for c in sc.mel_cases():
        inp = sc.cmn_inputs(c)
        got = _cmn(gpu, c, inp["mel"])
        w.add(got["mel"], sc.cmn_run(c, inp)["mel"], sc.cmn_bound(c, inp)["mel"], c)
        _same(got, _cmn(gpu, c, inp["mel"]), c)
        other = inp["mel"].copy()
        other[1:] = other[1:] * 3 + 1
        assert np.array_equal(_cmn(gpu, c, other)["mel"][0].view(np.uint32), got["mel"][0].view(np.uint32)), f"window 0 follows window 1: {c}"
    w.done()


@pytest.mark.parametrize("q", [0, 1, 80])
@pytest.mark.parametrize("B", [1, 3])
def test_log_cmn_gather_is_log_cmn_on_the_windows_rows(built_lib, gpu, q, B):
    for c in sc.mel_cases():
        T, NB = c["T"], c["NB"]
        rows = (B - 1) * q + T
        grid = sc.cmn_inputs(c, rows)["mel"]
        gb = Buf(gpu, rows, NB, grid).arm()                 # shared by the windows: read only
        fb = Buf(gpu, B * T, NB).arm(True)
        ops.log_cmn_gather(gb.v, fb.v, q=q, B=B, T=T, NB=NB, eps=sc.MEL_EPS)
        _finish([gb, fb], f"log_cmn_gather {c} q = {q} B = {B}")
        want = _cmn(gpu, c, np.stack([grid[b * q:b * q + T] for b in range(B)]))["mel"]
        assert np.array_equal(fb.get().reshape(B, T, NB).view(np.uint32), want.view(np.uint32)), f"{c} q = {q} B = {B}"


# ---- stem_conv ------------------------------------------------------------------------------------------------------------
def _stem(dev, NB, T, inp, z, fb=None):
    B, C = 3, sc.STEM_C
    fbb = Buf(dev, B * T, NB, (inp["fb"] if fb is None else fb).reshape(B * T, NB)).arm()
    chosen = list(range(B)) if z is None else z[0][:z[1]]
    mask = np.zeros((B, NB + 2, T + 2, C), bool)
    for b in chosen:
        mask[b, 1:-1, 1:-1] = True
    ib = Buf(dev, B * (NB + 2) * (T + 2), C).arm(mask.reshape(-1, C))
    am = Buf(dev, 1, B, np.zeros((1, B), F32)).arm(True)
    zl = zc = None
    if z is not None:
        zl, zc = _dev(np.array(z[0] + [0], np.int32), dev), _dev(np.array([z[1]], np.int32), dev)
    ops.stem_conv(fbb.v, _dev(inp["w"], dev), _dev(inp["bias"], dev), ib.v, B=B, T=T, NB=NB, C_out=C, amax=am.v, z_count=zc, z_list=zl)
    _finish([fbb, ib, am], f"stem_conv {NB} {T} {z}")
    return dict(img=ib.get().reshape(B, NB + 2, T + 2, C)[:, 1:-1, 1:-1], amax=am.get()[0]), chosen


def test_stem_conv(built_lib, gpu):
    w = Worst("stem_conv")
    for NB, T in sc.STEM:
        inp = sc.stem_inputs(NB, T)
        ref, bnd = sc.stem_run(NB, T, inp)["img"], sc.stem_bound(NB, T, inp)["img"]
        for z in sc.STEM_Z:
            got, chosen = _stem(gpu, NB, T, inp, z)
            want_amax = np.zeros(3, F32)
            for b in chosen:
                w.add(got["img"][b], ref[b], bnd[b], (NB, T, z))
                want_amax[b] = got["img"][b].max()
            assert np.array_equal(got["amax"], want_amax), f"tracker is not the maximum of the chosen images: {(NB, T, z)}"
            _same(got, _stem(gpu, NB, T, inp, z)[0], (NB, T, z))
        got, _ = _stem(gpu, NB, T, inp, None)
        alt, _ = _stem(gpu, NB, T, inp, None, _others(inp["fb"], 1))
        assert np.array_equal(alt["img"][0].view(np.uint32), got["img"][0].view(np.uint32))
    w.done()


# ---- stats_pool -----------------------------------------------------------------------------------------------------------
def _pool(dev, c, inp, img=None, masks=None):
    B, H, W, C, S, L = c["B"], c["H"], c["W"], c["C"], c["S"], c["L"]
    im = Buf(dev, B * (H + 2) * (W + 2), C)                  # the border keeps the NaN pattern: it is never read
    im.t.view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1] = _dev(inp["img"] if img is None else img, dev)
    im.arm()
    mb = Buf(dev, B * S, L, (inp["masks"] if masks is None else masks).reshape(B * S, L)).arm()
    sb = Buf(dev, B * S, 2 * C * H).arm(True)
    ops.stats_pool(im.v, mb.v, sb.v, B=B, H=H, W=W, C_in=C, S=S, L=L, active=_dev(inp["active"], dev))
    _finish([im, mb, sb], f"stats_pool {c}")
    return dict(stats=sb.get().reshape(B, S, 2 * C * H))


def test_stats_pool(built_lib, gpu):
    w = Worst("stats_pool")
    for c in sc.pool_cases():
        inp = sc.pool_inputs(c)
        got = _pool(gpu, c, inp)
        w.add(got["stats"], sc.pool_run(c, inp)["stats"], sc.pool_bound(c, inp)["stats"], c)
        _same(got, _pool(gpu, c, inp), c)
        if inp["active"] is None:
            alt = _pool(gpu, c, inp, _others(inp["img"], 1), _others(inp["masks"], 1))
            assert np.array_equal(alt["stats"][0].view(np.uint32), got["stats"][0].view(np.uint32)), f"window 0 follows window 1: {c}"
    w.done()


# ---- window_active, compact_active ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.ACTIVE_KINDS)
def test_window_active_and_compact_active_exact(built_lib, gpu, kind):
    g = np.random.default_rng(21)
    for B in sc.ACTIVE_B:
        want = sc.active_flags(B, kind)
        for per in (1, 300):
            m = np.zeros((B, per), F32)
            for b in np.nonzero(want)[0]:
                m[b, g.integers(per)] = g.choice([1.0, 1e-30, -2.0])
            mb = Buf(gpu, B, per, m).arm()
            fl = Buf(gpu, 1, B, dtype=torch.int32).arm(True)
            ops.window_active(mb.v, fl.v, B=B, per_window=per)
            _finish([mb, fl], f"window_active {B} {per}")
            assert np.array_equal(fl.get()[0], want)
        n = int(want.sum())
        fl = Buf(gpu, 1, B, want[None], dtype=torch.int32).arm()
        cnt = Buf(gpu, 1, 1, dtype=torch.int32).arm(True)
        lst = Buf(gpu, 1, B, dtype=torch.int32).arm(_cols(1, B, n))
        tot = Buf(gpu, 1, 2, np.zeros((1, 2), np.int64), dtype=torch.int64).arm(True)
        for _ in range(2):
            ops.compact_active(fl.v, cnt.v, lst.v, B=B, totals=tot.v)
        _finish([fl, cnt, lst, tot], f"compact_active {B} {kind}")
        assert int(cnt.get()[0, 0]) == n and np.array_equal(lst.get()[0, :n], np.nonzero(want)[0])
        assert tot.get()[0].tolist() == [2 * B, 2 * (B - n)], "totals do not accumulate over two calls"


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_what_they_cannot_serve(built_lib, gpu):
    """host-side argument checks: DZN_E_INVALID before anything is enqueued (the buffers are never touched)"""
    t = torch.zeros(4096, device=gpu)
    u8 = torch.zeros(4096, device=gpu, dtype=torch.uint8)
    bad = [
        ("ws_accum n % 4", lambda: ops.ws_accum(t, t, 1.0, True, 6)),
        ("ws_sum n % 4", lambda: ops.ws_sum([t], [1.0], t, 6)),
        ("ws_sum 41 sources", lambda: ops.ws_sum([t] * 41, [1.0] * 41, t, 4)),
        ("pad_rows D % 4", lambda: ops.pad_rows(t, t, B=1, L=2, Lp=4, pad=1, D=6)),
        ("stats_pool S W 4 > 64 KiB", lambda: ops.stats_pool(t, t, t, B=1, H=1, W=4097, C_in=4, S=4, L=4097)),
        ("glu_dwconv ks", lambda: ops.glu_dwconv(t, t, t, t, B=1, L=2, A=4, ks=9, ldu=8, ldo=4)),
        ("classify NC > 16", lambda: ops.classify(t, t, t, u8, rows=1, A=4, NC=17, S=2, ldz=4, logp=t)),
        ("classify S > 64", lambda: ops.classify(t, t, t, u8, rows=1, A=4, NC=2, S=65, ldz=4, logp=t)),
        ("groupnorm Cp % 4", lambda: ops.groupnorm_gelu(t, t, t, t, t, B=1, T=2, C=6, Cp=6, ld=8)),
        ("groupnorm ld % 4", lambda: ops.groupnorm_gelu(t, t, t, t, t, B=1, T=2, C=8, Cp=8, ld=10)),
        ("groupnorm Cp > 1024", lambda: ops.groupnorm_gelu(t, t, t, t, t, B=1, T=1, C=1028, Cp=1028, ld=1028)),
        ("stem_conv C % 4", lambda: ops.stem_conv(t, t, t, t, B=1, T=2, NB=2, C_out=6)),
        ("stem_conv 256 % (C / 4)", lambda: ops.stem_conv(t, t, t, t, B=1, T=2, NB=2, C_out=12)),
        ("frame_prep flen > 512", lambda: ops.frame_prep(t, t, t, B=1, stride=600, T=1, flen=513, fshift=160, Kp=520)),
    ]
    for what, call in bad:
        with pytest.raises(DznError, match="invalid argument"):      # `what` names the refusal in a failure's traceback
            call()
    torch.cuda.synchronize()
    assert not t.any() and not u8.any()
    # the largest request stats_pool still serves: S W 4 = 64 KiB exactly is not refused by the host check
    assert 4 * 4096 * 4 == 64 * 1024
