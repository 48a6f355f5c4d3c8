"""LN1's statistics from the FFN-down epilogue and the gate on the kept heads only (gate_heads_kernel, attention.hip; wiring in
engine.cpp seg_encoder_layer), at three levels.

Op level: ops.gate_heads against float64 inside bands, with the inputs, the reference and the per-element gate bound of
test_attention_matrix_gpu.py's gate_stats test.  What differs is where (mean, rstd) come from: P partial (sum, sum of squares)
pairs per row, each over n = C / P columns in fp32, added in double.  Their share of the bound, per row:
    e_mean = n u mean|x| + u |mean|                       (n - 1 adds per partial; the double sum adds nothing; one rounding to fp32)
    e_var  = (n + 1) u mean(x^2) + 2 |mean| em + em^2      (one product rounding + n - 1 adds per partial), em = n u mean|x|
    e_r    = 0.5 rv / (1 - rv) + 2 u, rv = e_var / (var + eps)      (|(1 + d)^-1/2 - 1| <= 0.5 |d| / (1 - |d|); sqrt and divide in
                                                                     double, one rounding to fp32)
and y = (x - mean) rstd gamma + beta in four roundings carries them as in that test.  The statistics themselves must be the bits
of stats_finalize_kernel on the same partials; columns of gate whose head is not kept keep their fill pattern.

Contraction level: what test_gemm_tiles_gpu.py leaves out for the FFN-down launch — residual + row statistics on the narrow tile
the dispatcher picks at N = 1024, with fewer K tiles than pipeline stages and an odd count, at M = 1 and either side of one row tile.

Engine level: a tiny pre-norm encoder whose six layers take every branch of the wiring (see _cfg), against the float64 oracle
and against an engine created under DZN_NO_EPILOGUE_STATS=1, with the launch counts per forward from the in-situ profiler.
"""
import os
from dataclasses import replace

import pytest
import torch

import _attn_cases as ac
import _gemm_cases as gc
import test_attention_matrix_gpu as am
import test_gemm_tiles_gpu as gt

pytestmark = pytest.mark.gpu

U = ac.U
EPS = 1e-5
ALL16 = tuple(range(16))
# kept-head lists per Htot: head 0 alone, the last head alone, a list with gaps, every head
KEPT = {1: [(0,)], 4: [(0,), (3,), (1, 2), (0, 1, 2, 3)], 16: [(0,), (15,), (1, 2, 4, 5, 6), ALL16]}
PS = (1, 8, 16, 32)


def _partials(x, P):
    """what a contraction epilogue with P wavefront tiles across the row leaves: fp32 (sum, sum of squares) of C / P columns each"""
    rows, C = x.shape
    xc = x.view(rows, P, C // P)
    return torch.stack([xc.sum(-1), (xc * xc).sum(-1)], dim=-1).contiguous()          # [rows, P, 2]


def _reference(x, gamma, beta, Wg, bg, cst, P):
    """(float64 gate [rows, Htot], its bound, the pre-activations, (mean, e_mean, rstd, e_r)) for statistics from P partials"""
    rows, C = x.shape
    Htot, n = C // 64, C // P
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    mabs, msq = xd.abs().mean(1, keepdim=True), (xd * xd).mean(1, keepdim=True)
    em = n * U * mabs
    e_mean = em + U * mean.abs()
    e_var = (n + 1) * U * msq + 2 * mean.abs() * em + em * em
    rv = e_var / (var + EPS)
    assert float(rv.max()) < 0.5
    e_r = 0.5 * rv / (1 - rv) + 2 * U
    dv = xd - mean
    yn = dv * rstd * gamma.double()
    y = yn + beta.double()
    ey = (rstd * gamma.double().abs()) * (e_mean + U * dv.abs()) + yn.abs() * (e_r + 2 * U) + U * y.abs()
    ref, bound, t = am._gate_ref(y.view(rows, Htot, 64), ey.view(rows, Htot, 64), Wg, bg, cst, 16)
    return ref, bound, t, (mean, e_mean, rstd, e_r)


def _run_gate_heads(gpu, name, x, xv, dvecs, kept, P, refs, problems):
    from diarizen_amd import ops
    rows, C = x.shape
    Htot = C // 64
    ref, bound, _, (mean, e_mean, rstd, e_r) = refs[P]
    part = _partials(x, P)
    pbuf, pview, phost = am._vec(gpu, part)
    hidx = torch.tensor(list(kept) + [99, 99], dtype=torch.int32, device=gpu)        # entries past h are never read
    gbuf, gview = am._out_band(gpu, rows, Htot)
    sbuf, sview = am._out_band(gpu, rows, 2)
    ops.gate_heads(xv, *dvecs, hidx, pview, out=(gview, sview), h=len(kept))
    want_st = ops.stats_finalize(pview, C)
    torch.cuda.synchronize()
    st = sview.cpu()
    if not torch.equal(am._bits(st), am._bits(want_st.cpu())):
        problems.append(f"{name}: (mean, rstd) are not the bits of stats_finalize on the same partials")
    if not torch.isfinite(st).all():
        problems.append(f"{name}: stats not finite")
    else:
        if not bool(((st[:, :1].double() - mean).abs() <= e_mean).all()):
            problems.append(f"{name}: mean outside its bound")
        if not bool((((st[:, 1:].double() - rstd) / rstd).abs() <= e_r).all()):
            problems.append(f"{name}: rstd outside its bound")
    got = gview.cpu()
    k = list(kept)
    r = am._check_gate(name, got[:, k], ref[:, k], bound[:, k], problems)
    other = [H for H in range(Htot) if H not in kept]
    if other and not bool((got[:, other].view(torch.int32) == ac.PATTERN).all()):
        problems.append(f"{name}: a gate column of a head that is not kept was written")
    if not am._band_intact(gbuf, rows, Htot):
        problems.append(f"{name}: a band of gate changed")
    if not am._band_intact(sbuf, rows, 2):
        problems.append(f"{name}: a band of stats changed")
    if not am._same_bits(pbuf, phost):
        problems.append(f"{name}: the partials changed")
    return r


@pytest.mark.parametrize("loud", [False, True], ids=["offset", "saturating"])
@pytest.mark.parametrize("rows", am.GATE_ROWS)
@pytest.mark.parametrize("Htot", [1, 4, 16])
def test_gate_heads_against_float64_inside_bands(built_lib, gpu, Htot, rows, loud):
    """every kept-head list x every partial count P (at the largest row count: list i with P i), row stride Htot 64 + 8 with NaN
    pad columns and NaN band rows, PATTERN-filled gate and stats"""
    problems = []
    C = Htot * 64
    x, gamma, beta, Wg, bg, cst = am._gate_inputs(rows, Htot, loud, True)
    xb, xv, xh = am._in2d(gpu, x, C + 8)
    dvecs = [am._vec(gpu, t)[1] for t in (gamma, beta, Wg, bg, cst)]
    refs = {P: _reference(x, gamma, beta, Wg, bg, cst, P) for P in PS}
    if loud:
        assert float(refs[1][2].abs().max()) > 89.0
    lists = KEPT[Htot]
    combos = [(k, P) for k in lists for P in PS] if rows <= 203 else [(lists[i % len(lists)], P) for i, P in enumerate(PS)]
    worst = 0.0
    for kept, P in combos:
        name = f"gate_heads Htot={Htot} rows={rows} {'saturating' if loud else 'offset'} kept={kept} P={P}"
        worst = max(worst, _run_gate_heads(gpu, name, x, xv, dvecs, kept, P, refs, problems))
    print(f"[gate_heads Htot={Htot} rows={rows} {'saturating' if loud else 'offset'}] worst error / bound {worst:.3f}")
    if not am._same_bits(xb, xh):
        problems.append("the input changed")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("Htot,kept", [(1, (0,)), (4, (0, 3))])
def test_gate_heads_wavefronts_walk_several_passes_of_many_rows(built_lib, gpu, Htot, kept):
    """a wavefront takes 16 / h rows per pass and at most 4096 wavefronts are launched: 70001 rows are 4376 passes of 16 rows
    (h = 1) and 8751 passes of 8 (h = 2), so wavefronts walk a second and a third pass, the last pass ragged"""
    problems = []
    rows = 70001
    x, gamma, beta, Wg, bg, cst = am._gate_inputs(rows, Htot, False, True)
    xb, xv, xh = am._in2d(gpu, x, Htot * 64 + 8)
    dvecs = [am._vec(gpu, t)[1] for t in (gamma, beta, Wg, bg, cst)]
    refs = {8: _reference(x, gamma, beta, Wg, bg, cst, 8)}
    _run_gate_heads(gpu, f"gate_heads Htot={Htot} rows={rows} kept={kept}", x, xv, dvecs, kept, 8, refs, problems)
    assert am._same_bits(xb, xh) and not problems, "\n".join(problems)


def test_gate_heads_rows_without_16_byte_alignment(built_lib, gpu):
    """row stride Htot 64 + 9: the rows are not 16-byte aligned, the kernel's scalar-load form runs"""
    problems = []
    rows, Htot = 5, 16
    x, gamma, beta, Wg, bg, cst = am._gate_inputs(rows, Htot, False, True)
    xb, xv, xh = am._in2d(gpu, x, Htot * 64 + 9)
    dvecs = [am._vec(gpu, t)[1] for t in (gamma, beta, Wg, bg, cst)]
    refs = {16: _reference(x, gamma, beta, Wg, bg, cst, 16)}
    _run_gate_heads(gpu, "gate_heads odd stride", x, xv, dvecs, (1, 2, 4, 5, 6), 16, refs, problems)
    assert am._same_bits(xb, xh) and not problems, "\n".join(problems)


def test_gate_heads_refuses_invalid_counts_before_any_launch(built_lib, gpu):
    """h < 1, h > Htot, Htot > 16, P < 1, P > 32: DZN_E_INVALID, and neither output is touched"""
    from diarizen_amd import _lib, ops
    rows = 3

    def attempt(Htot, h, P):
        g = torch.Generator().manual_seed(Htot)
        C = Htot * 64
        x = torch.randn(rows, C, generator=g).to(gpu)
        vecs = [torch.randn(n, generator=g).to(gpu) for n in (C, C, 8 * 64, 8, Htot)]
        hidx = torch.zeros(32, dtype=torch.int32, device=gpu)
        part = torch.zeros(rows, 40, 2, device=gpu)
        gbuf, gview = am._out_band(gpu, rows, Htot)
        sbuf, sview = am._out_band(gpu, rows, 2)
        with pytest.raises(_lib.DznError, match="invalid argument"):
            ops.gate_heads(x, *vecs, hidx, part, out=(gview, sview), h=h, P=P)
        torch.cuda.synchronize()
        assert bool((gbuf.cpu() == ac.PATTERN).all()) and bool((sbuf.cpu() == ac.PATTERN).all()), (Htot, h, P)

    attempt(4, 0, 8)
    attempt(4, 5, 8)
    attempt(17, 3, 8)
    attempt(4, 2, 0)
    attempt(4, 2, 33)


# ---- contraction level ----
@pytest.mark.parametrize("M", [1, 127, 129])
@pytest.mark.parametrize("K", [32, 64, 96])
def test_residual_and_row_statistics_on_the_short_k_tile(built_lib, gpu, monkeypatch, M, K):
    """the FFN-down launch of a heavily pruned layer: residual + stat_partial at N = 1024 on the 128 x 64 tile the f32h dispatcher
    picks for K <= 512, with one, two and three 32-column K tiles; test_gemm_tiles_gpu.py's checks, its statistics bound included
    (against float64 of the C rows that were stored)"""
    monkeypatch.setitem(gc.FEATURES, "FRS", dict(R=True, stats=True))
    gt.run_twice(gpu, "f32h", None, M, 1024, K, "FRS", 99, geom=(128, 64, 4, 1))


# ---- engine level ----
# layer:  0 attention + FFN, input from the positional conv            -> gate_stats (the pass over whole rows)
#         1 attention after an FFN, kept heads 0 and 3 (first and last) -> gate_heads
#         2 no attention, after an FFN                                 -> statistics finalized behind layer 1's FFN-down, no row_stats
#         3 attention after the attention-less layer, no FFN of its own -> gate_heads
#         4 attention after a layer without FFN                        -> gate_stats
#         5 attention after an FFN, one head                           -> gate_heads
def _cfg():
    from diarizen_amd.configs import TINY_LN
    return replace(TINY_LN, name="tiny_ln_stats", remaining_heads=((0, 3), (0, 3), (), (2,), (0, 1, 3), (1,)),
                   ffn_dims=(100, 77, 40, 0, 129, 64))


B_, N_ = 3, 16000


@pytest.fixture(scope="module")
def engines(built_lib, gpu):
    """{"default" | "off": (logp, multilabel, launches per class of one forward, logp of window 1 launched alone)} + the float64
    reference; "off" = an engine created under DZN_NO_EPILOGUE_STATS=1"""
    from diarizen_amd import _lib
    from diarizen_amd.engine import Engine
    from oracle import seg_model
    from oracle.gen_golden import synth_wave
    cfg = _cfg()
    # seeded weights of the same model with an FFN in layer 3, whose tensors then shrink to width 0 for the oracle (with a zero
    # output bias its FFN adds nothing); the engine is not given them at all
    sd = dict(seg_model.seg_state_dict(replace(cfg, ffn_dims=(100, 77, 40, 8, 129, 64)), 0))
    ffn3 = "wavlm_model.encoder.transformer.layers.3.feed_forward."
    D = cfg.embed_dim
    sd.update({ffn3 + "intermediate_dense.weight": torch.zeros(0, D), ffn3 + "intermediate_dense.bias": torch.zeros(0),
               ffn3 + "output_dense.weight": torch.zeros(D, 0), ffn3 + "output_dense.bias": torch.zeros(D)})
    wave = synth_wave(B_, N_, 7)
    ref = seg_model.seg_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, cfg, wave.double())
    out = {"ref": ref, "ref_ml": seg_model.to_multilabel(ref.float(), cfg).to(torch.uint8), "L": ref.shape[1]}
    esd = {k: v for k, v in sd.items() if not k.startswith(ffn3)}
    for key, off in (("default", False), ("off", True)):
        old = os.environ.pop("DZN_NO_EPILOGUE_STATS", None)
        if off:
            os.environ["DZN_NO_EPILOGUE_STATS"] = "1"
        try:
            eng = Engine(cfg, esd, max_batch=B_, max_samples=N_, precision="f32h", device=gpu)
        finally:
            os.environ.pop("DZN_NO_EPILOGUE_STATS", None)
            if old is not None:
                os.environ["DZN_NO_EPILOGUE_STATS"] = old
        w = wave.to(gpu)
        eng.segment(w)                                   # tables are built on the first call
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        try:
            logp, ml = eng.segment(w)
            torch.cuda.synchronize()
            launches = {p["name"]: p["launches"] for p in _lib.profile_collect()}
        finally:
            _lib.profile_enable(False)
        one, one_ml = eng.segment(w[1:2].contiguous())
        torch.cuda.synchronize()
        out[key] = (logp.cpu(), ml.cpu(), launches, one.cpu(), one_ml.cpu())
        eng.close()
    return out


@pytest.mark.parametrize("key", ["default", "off"])
def test_engine_holds_the_strict_bar_with_and_without_epilogue_statistics(engines, key):
    """max |logp - float64 oracle| <= 1e-3 and the oracle's decisions; B = 3 windows of 49 frames: 147 rows, not a multiple of 128"""
    logp, ml = engines[key][:2]
    assert (B_ * engines["L"]) % 128 != 0
    err = (logp.double() - engines["ref"]).abs().max().item()
    print(f"[encoder stats] {key}: max |logp - oracle| = {err:.3e}")
    assert err <= 1e-3
    assert torch.equal(ml, engines["ref_ml"])


@pytest.mark.parametrize("key", ["default", "off"])
def test_window_alone_equals_window_in_batch(engines, key):
    logp, ml, _, one, one_ml = engines[key]
    assert torch.equal(one[0], logp[1]) and torch.equal(one_ml[0], ml[1])


def test_launch_counts_per_forward(engines):
    """gate_stats (class gate_ln_stats) exactly for layers 0 and 4, gate_heads for layers 1, 3 and 5, one finalize per out_proj
    in front of an FFN (layers 0, 1, 4, 5) + one behind layer 1's FFN-down; row_stats only where no producer can supply the
    statistics: the feature projection and the four folded LayerNorms of each Conformer layer.  Under DZN_NO_EPILOGUE_STATS=1:
    gate_stats for all five attention layers, row_stats in front of all five FFNs as well, no finalize, no gate_heads."""
    conf = 1 + 4 * _cfg().conf_layers
    d, o = engines["default"][2], engines["off"][2]
    assert (d.get("gate_ln_stats", 0), d.get("gate_heads", 0), d.get("stats_finalize", 0), d.get("row_stats", 0)) == (2, 3, 5, conf), d
    assert (o.get("gate_ln_stats", 0), o.get("gate_heads", 0), o.get("stats_finalize", 0), o.get("row_stats", 0)) == (5, 0, 0, conf + 5), o
    assert d.get("gate", 0) == 0 and o.get("gate", 0) == 0
