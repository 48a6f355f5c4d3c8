"""Kernel-level matrix of the attention family (attention.hip, attention_split.hip, attention_planes.hip with its packing
kernel) and of the gate kernels that feed its bias: every form, addressed by entry point, with and without the gated
relative-position bias, at the lengths where the indexing is decided (1; the 16-query block, the 64-key tile and the 128-query
workgroup +- 1; 399; 798), head counts from 1 to dense, and input classes that make a softmax error visible.  tests/_attn_cases.py
holds the case table, the inputs, the float64 reference and the DERIVED per-element bound (test_attention_bounds_host.py shows on
the CPU that an ideal kernel keeps a factor 4 under it).

Per launch: (1) every stored element within ITS OWN bound of float64 — per element, never against a global maximum; (2) every
buffer sits inside a larger allocation whose bands are compared bit for bit afterwards (qkv, gate, table, amax: NaN bands and, in
the strided variant, NaN pad columns, so a read outside the logical operand poisons the result; out: a fixed NaN bit pattern; the
planes / scale scratch: its documented zero tail of 64 rows, then bands of fp16 / fp32 NaN); (3) every stored element finite;
(4) a second identical launch gives identical bits; (5) schedule forms are not arithmetic: the three (qb, pf) forms of the
planes kernel and the noskip form of the split kernels give the bits of the shipped form; (6) window b of a batched launch
equals the same window launched alone, bit for bit (D1 and D4: for the planes kernel D4 is the test that the next window's loud
masked rows change nothing); (7) permuting the head slots and head_idx permutes the output, bit for bit; (8) the all-zero window
of D6a gives exact zeros, the constant V of D6b its vector.

The worst error / bound ratio per (form, bias, class, L) goes to attention_matrix.json, beside the report of
test_gemm_tiles_gpu.py (DZN_REPORT_DIR overrides the directory).
"""
import json
import os
import re

import pytest
import torch

import _attn_cases as ac

pytestmark = pytest.mark.gpu

G = ac.GUARD_ROWS
NAN = float("nan")
H16_NAN = 0x7E00                # fp16 NaN: what the bands of the planes scratch hold
_REPORT = {}


def _report_dir():
    """the suite's report directory: where test_f32h_grade_gpu.py writes its report (test_gemm_tiles_gpu.py's logic)"""
    if os.environ.get("DZN_REPORT_DIR"):
        return os.environ["DZN_REPORT_DIR"]
    src = open(os.path.join(os.path.dirname(__file__), "test_f32h_grade_gpu.py")).read()
    return re.search(r'os\.makedirs\("([^"]+)"', src).group(1)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if _REPORT:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        form = {}
        for k, v in _REPORT.items():
            f = k.split("/")[0]
            form[f] = max(form.get(f, 0.0), v)
        json.dump({"worst_ratio_per_form": form, "worst_ratio": dict(sorted(_REPORT.items())),
                   "note": "max over elements of |kernel - float64 reference| / derived bound (tests/_attn_cases.py), per "
                           "form/bias/class/L; > 1 fails"},
                  open(os.path.join(out, "attention_matrix.json"), "w"), indent=1)


# ---- buffers inside bands ----
def _in2d(dev, data, ld, fill=NAN, tail_rows=0, tail_fill=0.0):
    """data [rows, cols] at row stride ld inside G band rows either side (and `tail_rows` rows of tail_fill after the data):
    (whole flat device buffer, the logical strided view, a host copy of the whole buffer)"""
    rows, cols = data.shape
    host = torch.full(((G + rows + tail_rows + G), ld), fill, dtype=data.dtype)
    host[G:G + rows, :cols] = data
    if tail_rows:
        host[G + rows:G + rows + tail_rows] = tail_fill
    buf = host.reshape(-1).to(dev)
    return buf, buf[G * ld:].as_strided((rows, cols), (ld, 1)), host.reshape(-1)


def _vec(dev, data, pad=64, fill=NAN):
    host = torch.full((data.numel() + 2 * pad,), fill, dtype=data.dtype)
    host[pad:pad + data.numel()] = data.reshape(-1)
    buf = host.to(dev)
    return buf, buf[pad:pad + data.numel()].view(data.shape), host


def _same_bits(dev_buf, host):
    a, b = dev_buf.cpu(), host
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


class _Launch:
    """one set of device buffers for (inputs of a launch, strides): out preset to PATTERN, the planes scratch zero-filled, every
    buffer in bands; run(form) launches, read() returns the stored elements and notes every band that changed"""

    def __init__(self, dev, qkv, gate, table, heads, amax, B, L, h, Htot, ldqkv, ldo):
        self.dev, self.B, self.L, self.h, self.Htot, self.ldo = dev, B, L, h, Htot, ldo
        rows = B * L
        self.qkv_buf, self.qkv, self.qkv_host = _in2d(dev, qkv, ldqkv)
        self.kw = {}
        self.inputs = [("qkv", self.qkv_buf, self.qkv_host)]
        if heads is not None:
            gb, gv, gh = _in2d(dev, gate, Htot)
            tb, tv, th = _vec(dev, table)
            self.kw = dict(gate=gv, table=tv, head_idx=torch.tensor(heads, dtype=torch.int32, device=dev), Htot=Htot)
            self.inputs += [("gate", gb, gh), ("table", tb, th)]
        ab, self.amax, ah = _vec(dev, amax, pad=4)
        self.inputs.append(("amax", ab, ah))
        self.out_buf = torch.full(((G + rows + G) * ldo,), ac.PATTERN, dtype=torch.int32, device=dev)
        self.out = self.out_buf.view(torch.float32)[G * ldo:].as_strided((rows, h * 64), (ldo, 1))
        self.idx = ((G + torch.arange(rows))[:, None] * ldo + torch.arange(h * 64)[None, :]).reshape(-1)
        self.planes_buf = self.kvs_buf = None

    def _scratch(self):
        rows, kv_ld = self.B * self.L + 64, 2 * self.h * 64
        host = torch.full((G * kv_ld + 2 * rows * kv_ld + G * kv_ld,), H16_NAN, dtype=torch.int16)
        host[G * kv_ld:G * kv_ld + 2 * rows * kv_ld] = 0
        self.planes_host, self.planes_buf = host, host.to(self.dev)
        self.planes = self.planes_buf[G * kv_ld:G * kv_ld + 2 * rows * kv_ld].view(2, rows, kv_ld)
        self.kvs_buf, kv, self.kvs_host = _in2d(self.dev, torch.zeros(rows, 2 * self.h), 2 * self.h)
        self.kvs = kv

    def run(self, form):
        from diarizen_amd import _lib, ops
        self.out_buf.fill_(ac.PATTERN)
        common = dict(out=self.out, **self.kw)
        if form == "planes":
            self._scratch()
            ops.attention_planes(self.qkv, self.B, self.L, self.h, amax=self.amax, planes=self.planes, kvs=self.kvs, **common)
        elif form == "f32h_split":
            ops.attention(self.qkv, self.B, self.L, self.h, precision=_lib.DZN_PREC_F32_H2, amax=self.amax, **common)
        else:
            prec = _lib.DZN_PREC_F32 if form == "f32" else _lib.DZN_PREC_F32_SPLIT
            ops.attention(self.qkv, self.B, self.L, self.h, precision=prec, **common)
        torch.cuda.synchronize()
        return self

    def read(self, what, problems):
        """stored elements [B L, h 64] as fp32 (host); every band and every input compared bit for bit"""
        hbuf = self.out_buf.cpu()
        vals = hbuf[self.idx].view(torch.float32).view(self.B * self.L, self.h * 64)
        band = hbuf.clone()
        band[self.idx] = ac.PATTERN
        bad = (band != ac.PATTERN).nonzero().reshape(-1)
        if bad.numel():
            first = int(bad[0])
            problems.append(f"{what}: {bad.numel()} band elements of out changed, first at row {first // self.ldo - G}, col "
                            f"{first % self.ldo} (rows from the logical origin, ldo {self.ldo})")
        for name, buf, host in self.inputs:
            if not _same_bits(buf, host):
                problems.append(f"{what}: input buffer {name} changed")
        if self.planes_buf is not None:
            rows, kv_ld = self.B * self.L + 64, 2 * self.h * 64
            hp = self.planes_buf.cpu()
            lo, hi = G * kv_ld, G * kv_ld + 2 * rows * kv_ld
            if not (torch.equal(hp[:lo], self.planes_host[:lo]) and torch.equal(hp[hi:], self.planes_host[hi:])):
                problems.append(f"{what}: a band of the planes scratch changed")
            if hp[lo:hi].view(2, rows, kv_ld)[:, rows - 64:].any():
                problems.append(f"{what}: the zero tail of the planes scratch was written")
            hk = self.kvs_buf.cpu().view(-1, 2 * self.h)
            keep = torch.ones(hk.shape[0], dtype=torch.bool)
            keep[G:G + self.B * self.L] = False
            if not torch.equal(hk[keep].view(torch.int32), self.kvs_host.view(-1, 2 * self.h)[keep].view(torch.int32)):
                problems.append(f"{what}: the zero tail or a band of the scale scratch changed")
        return vals


def _launch_of(dev, inp, strided_ld, windows=None, perm=None):
    """buffers for the case's inputs; windows = [b]: that window alone (B = 1, its own amax); perm: head slots permuted"""
    B, L, h, Htot, heads = inp["B"], inp["L"], inp["h"], inp["Htot"], inp["heads"]
    qkv, gate, amax = inp["qkv"], inp["gate"], inp["amax"]
    if windows is not None:
        (b,) = windows
        qkv, amax, B = qkv[b * L:(b + 1) * L], amax[b:b + 1], 1
        gate = gate[b * L:(b + 1) * L] if gate is not None else None
    if perm is not None:
        qkv = qkv.view(-1, 3, h, 64)[:, :, perm].reshape(-1, 3 * h * 64)
        heads = [heads[j] for j in perm] if heads is not None else None
    ldqkv, ldo = strided_ld
    return _Launch(dev, qkv.contiguous(), gate, inp["table"], heads, amax, B, L, h, Htot, ldqkv, ldo)


def _set_planes(qb, pf):
    from diarizen_amd import _lib
    lib = _lib.load()
    lib.dzn_op_set_attention_qb(qb)
    lib.dzn_op_set_attention_prefetch(pf)


def _bits(x):
    return x.view(torch.int32)


def _case_id(c):
    return f"{c[1]}-{c[2]}-{c[3]}-L{c[4]}" + ("-strided" if c[5] else "")


_MATRIX = [(i, f, s, c, L, st) for i, (s, L, c, st) in enumerate(ac.cases()) for f in ac.FORMS]


@pytest.mark.parametrize("case", _MATRIX, ids=_case_id)
def test_attention_form_within_its_bound_inside_bands(built_lib, gpu, case):
    from diarizen_amd import _lib
    _, form, shape, cls, L, strided = case
    inp, ref = ac.make_inputs(shape, L, cls), ac.launch_ref(shape, L, cls)
    B, h = inp["B"], inp["h"]
    ld = ac.strides(shape, strided)
    problems = []
    coord = f"{form} {shape} L={L} {cls}" + (" strided" if strided else "")
    la = _launch_of(gpu, inp, ld)
    got = la.run(form).read(coord, problems)

    # (3) finite, (1) per-element bound
    assert torch.isfinite(got).all(), f"{coord}: {int((~torch.isfinite(got)).sum())} stored elements are not finite (or were never stored)"
    bound, _ = ac.bound_of(ref, form)
    err = (got.double() - ref["out"]).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    key = f"{form}/{'bias' if ac.has_bias(shape) else 'nobias'}/{cls}/L{L}"
    _REPORT[key] = max(_REPORT.get(key, 0.0), worst)
    print(f"[attention matrix {coord}] worst error / bound {worst:.3f}")
    if worst > 1.0:
        at = int(ratio.argmax())
        r, c = at // (h * 64), at % (h * 64)
        problems.append(f"{coord}: error / bound = {worst:.3f} at window {r // L}, query {r % L}, head slot {c // 64}, d {c % 64}: "
                        f"got {float(got[r, c])!r}, float64 {float(ref['out'][r, c])!r}, bound {float(bound[r, c]):.3e}; "
                        f"{int((ratio > 1).sum())} elements over their bound")

    # (8) the degenerate classes, stated outright
    if cls == "D6a":
        zero = got.view(B, -1)[0]
        if not bool((_bits(zero) == 0).all() or (zero == 0).all()):
            problems.append(f"{coord}: the all-zero window does not give exact zeros")
    if cls == "D6b":
        vec = inp["qkv"].view(B, L, -1)[:, :, 2 * h * 64:].reshape(B * L, h * 64).double()
        if not bool(((got.double() - vec).abs() <= bound).all()):
            problems.append(f"{coord}: constant V rows do not come back within the bound")

    # (4) a second identical launch
    again = la.run(form).read(coord + " (second launch)", problems)
    if not torch.equal(_bits(again), _bits(got)):
        problems.append(f"{coord}: a second identical launch differs in {int((_bits(again) != _bits(got)).sum())} elements")

    # (5) schedule forms are not arithmetic
    if form == "planes":
        for qb, pf in ac.PLANES_SCHEDULES[1:]:
            try:
                _set_planes(qb, pf)
                other = la.run(form).read(f"{coord} qb={qb} pf={pf}", problems)
            finally:
                _set_planes(1, 1)
            if not torch.equal(_bits(other), _bits(got)):
                problems.append(f"{coord}: schedule form qb={qb} pf={pf} differs from the shipped form in "
                                f"{int((_bits(other) != _bits(got)).sum())} elements")
    if form in ("f32s", "f32h_split"):
        lib = _lib.load()
        try:
            lib.dzn_op_set_attention_noskip(1)
            full = la.run(form).read(coord + " noskip", problems)
        finally:
            lib.dzn_op_set_attention_noskip(0)
        if not torch.equal(_bits(full), _bits(got)):
            problems.append(f"{coord}: the noskip form differs in {int((_bits(full) != _bits(got)).sum())} elements")

    # (6) batch independence
    if cls in ("D1", "D4") and B >= 2:
        for b in (range(B) if B <= 3 else sorted({0, 1, 7, 8, B - 1} & set(range(B)))):
            alone = _launch_of(gpu, inp, ld, windows=[b]).run(form).read(f"{coord} window {b} alone", problems)
            if not torch.equal(_bits(alone), _bits(got[b * L:(b + 1) * L])):
                problems.append(f"{coord}: window {b} launched alone differs from the batched launch in "
                                f"{int((_bits(alone) != _bits(got[b * L:(b + 1) * L])).sum())} elements")

    # (7) head independence
    if cls == "D1" and h >= 2:
        perm = list(range(1, h)) + [0] if h == 2 else [(3 * j + 1) % h for j in range(h)] if h % 3 else list(reversed(range(h)))
        assert sorted(perm) == list(range(h)) and perm != list(range(h))
        moved = _launch_of(gpu, inp, ld, perm=perm).run(form).read(f"{coord} heads permuted", problems)
        want = got.view(B * L, h, 64)[:, perm].reshape(B * L, h * 64)
        if not torch.equal(_bits(moved), _bits(want)):
            problems.append(f"{coord}: permuting the head slots does not permute the output "
                            f"({int((_bits(moved) != _bits(want)).sum())} elements differ)")
    assert not problems, "\n".join(problems)


# ---- the gate kernels ----
GATE_ROWS = (1, 3, 5, 203, 2 * 8192 + 7)        # the last: every wavefront of gate_stats_kernel walks more than one row, last round partial
U = ac.U


def _gate_inputs(rows, Htot, loud, ln):
    g = torch.Generator().manual_seed(1009 * Htot + rows + (1 if loud else 0) + (2 if ln else 0))
    C = Htot * 64
    x = torch.randn(rows, C, generator=g) * 2.5 + torch.randn(rows, 1, generator=g) * 10.0     # common offset 4 x the spread
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    Wg, bg = torch.randn(8, 64, generator=g) * 0.2, torch.randn(8, generator=g)
    cst = torch.rand(Htot, generator=g) + 0.5
    if loud:                                   # pre-activations that reach +-90: both sigmoids saturate
        y = torch.nn.functional.layer_norm(x.double(), (C,), gamma.double(), beta.double()) if ln else x.double()
        t = (y.view(rows, Htot, 64) @ Wg.double().T + bg.double()).view(rows, Htot, 2, 4).sum(-1)
        c = 90.0 / float(t.abs().max())
        Wg, bg = (Wg * c).float(), (bg * c).float()
    return x, gamma, beta, Wg, bg, cst


def _gate_ref(y, ey, Wg, bg, cst, nterms):
    """float64 gate of rows y [rows, Htot, 64] whose elements carry the error ey, and its per-element bound: a dot of `nterms` fp32
    steps (+ 2 for the pre-summed weights of gate_stats_kernel, which the 8 x 64 form does not have but which cost it two more
    adds), two sigmoids (slope <= 1/4; expf 1 ulp, one add, one divide: 6 u relative with room for the divide), the final
    ga * (gb * cst - 1) + 2 in four roundings"""
    W, b = Wg.double(), bg.double()
    t = (y @ W.T + b).view(*y.shape[:2], 2, 4).sum(-1)                                         # [rows, Htot, 2]
    Wabs = W.abs().view(2, 4, 64).sum(1)                                                         # [2, 64]
    dt = ey @ Wabs.T + (nterms + 5) * U * (y.abs() @ Wabs.T + b.abs().view(2, 4).sum(1))
    sg = torch.sigmoid(t)
    es = 0.25 * dt + 6 * U * sg
    ga, gb, ea, eb = sg[..., 0], sg[..., 1], es[..., 0], es[..., 1]
    c = cst.double()
    inner = gb * c - 1.0
    ref = ga * inner + 2.0
    bound = eb * c.abs() * ga + ea * inner.abs() + U * ga * ((gb * c).abs() + inner.abs()) + U * (ga * inner).abs() + U * ref.abs()
    return ref, bound, t


def _check_gate(name, got, ref, bound, problems):
    if not torch.isfinite(got).all():
        problems.append(f"{name}: not finite")
        return 0.0
    ratio = float(((got.double() - ref).abs() / bound).max())
    if ratio > 1.0:
        problems.append(f"{name}: error / bound = {ratio:.3f}")
    return ratio


def _out_band(dev, rows, cols):
    buf = torch.full(((G + rows + G) * cols,), ac.PATTERN, dtype=torch.int32, device=dev)
    return buf, buf.view(torch.float32)[G * cols:(G + rows) * cols].view(rows, cols)


def _band_intact(buf, rows, cols):
    h = buf.cpu()
    return bool((h[:G * cols] == ac.PATTERN).all() and (h[(G + rows) * cols:] == ac.PATTERN).all())


@pytest.mark.parametrize("loud", [False, True], ids=["offset", "saturating"])
@pytest.mark.parametrize("rows", GATE_ROWS)
@pytest.mark.parametrize("Htot", [1, 4, 12, 16])
def test_gate_kernels_against_float64_inside_bands(built_lib, gpu, Htot, rows, loud):
    """ops.gate on given rows and ops.gate_stats on raw rows (LayerNorm in registers), row stride ldx = Htot 64 + 8 with NaN pad
    columns, NaN band rows around the input, PATTERN bands around gate and stats.  The LayerNorm's share of the bound: the mean
    is a sum of C = Htot 64 terms in 16 + 6 steps and a divide (23 u mean|x|), the variance likewise on the centred values, rstd
    one sqrt and one divide; y = (x - mean) rstd gamma + beta in four roundings."""
    from diarizen_amd import ops
    problems = []
    C = Htot * 64
    ldx = C + 8
    for ln in (False, True):
        x, gamma, beta, Wg, bg, cst = _gate_inputs(rows, Htot, loud, ln)
        xb, xv, xh = _in2d(gpu, x, ldx)
        dW, db, dc = (_vec(gpu, t)[1] for t in (Wg, bg, cst))
        gbuf, gview = _out_band(gpu, rows, Htot)
        name = f"{'gate_stats' if ln else 'gate'} Htot={Htot} rows={rows} {'saturating' if loud else 'offset'}"
        if not ln:
            ops.gate(xv, dW, db, dc, out=gview)
            torch.cuda.synchronize()
            ref, bound, t = _gate_ref(x.double().view(rows, Htot, 64), torch.zeros(rows, Htot, 64, dtype=torch.float64), Wg, bg, cst, 64)
        else:
            sbuf, sview = _out_band(gpu, rows, 2)
            ops.gate_stats(xv, _vec(gpu, gamma)[1], _vec(gpu, beta)[1], dW, db, dc, out=(gview, sview))
            torch.cuda.synchronize()
            xd = x.double()
            mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + 1e-5)
            e_mean = 23 * U * xd.abs().mean(1, keepdim=True)
            dv = xd - mean
            e_r = 0.5 * (2 * e_mean * rstd + 27 * U) + 3 * U                   # relative error of rstd
            yn = dv * rstd * gamma.double()
            y = yn + beta.double()
            ey = (rstd * gamma.double().abs()) * (e_mean + U * dv.abs()) + yn.abs() * (e_r + 2 * U) + U * y.abs()
            ref, bound, t = _gate_ref(y.view(rows, Htot, 64), ey.view(rows, Htot, 64), Wg, bg, cst, 16)
            st = sview.cpu()
            if not torch.isfinite(st).all():
                problems.append(f"{name}: stats not finite")
            else:
                if not bool(((st[:, :1].double() - mean).abs() <= e_mean + U * mean.abs()).all()):
                    problems.append(f"{name}: mean outside its bound")
                if not bool((((st[:, 1:].double() - rstd) / rstd).abs() <= e_r).all()):
                    problems.append(f"{name}: rstd outside its bound")
            if not torch.equal(_bits(ops.row_stats(xv).cpu()), _bits(st)):
                problems.append(f"{name}: stats differ from ops.row_stats")
            if not _band_intact(sbuf, rows, 2):
                problems.append(f"{name}: a band of stats changed")
        if loud:
            assert float(t.abs().max()) > 89.0
        r = _check_gate(name, gview.cpu(), ref, bound, problems)
        print(f"[{name}] worst error / bound {r:.3f}")
        if not _band_intact(gbuf, rows, Htot):
            problems.append(f"{name}: a band of gate changed")
        if not _same_bits(xb, xh):
            problems.append(f"{name}: the input changed")
    assert not problems, "\n".join(problems)
