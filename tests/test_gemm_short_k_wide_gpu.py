"""The wide tile of the short-K f32h contractions (launch_gemm_split_np: N >= 512 and 128 <= K <= 512 — the out-projections
and the narrow FFN-down launches of the pruned encoder), at four levels.

Forced by name: the tile on test_gemm_tiles_gpu.py's six checks (run_twice) at its own edges — one row, one row short of a row
tile, 17 rows into the second; a column tile plus one float4, 12 and 13 columns short of two tiles (the last with odd strides:
the scalar epilogue) — with K = 128, 160 and 512 (4, 5 and 16 K tiles: an even and an odd count, the shortest and the longest
launch the rule sends here) and four feature sets.  The bounds are _gemm_cases' derived per-element bound and run_case's
statistics bound; nothing is tuned here.

Automatic dispatch, through the profiler class: the rule's two ends, its two neighbours, at M = 1 and M = 129 alike (the rule
must not follow M: a partial is the sum over one wavefront tile's columns, so a tile that followed M would make a window's
float outputs depend on its batch).  Every case carries residual + row statistics, as the FFN-down launch does.

Batch invariance: the first 129 rows of an M = 1000 launch against the M = 129 launch of the same rows, bit for bit.

Partials: the launch leaves 8 per row at N = 1024 (gemm_stat_partials_last, and the layout of the partial buffer itself);
gate_heads on them against float64 of the stored rows at test_encoder_stats_gpu.py's bound for P = 8, and against gate_stats on
the same rows at the sum of the two kernels' bounds.
"""
import ctypes

import pytest
import torch

import _gemm_cases as gc
import test_attention_matrix_gpu as am
import test_encoder_stats_gpu as es
import test_gemm_tiles_gpu as gt

pytestmark = pytest.mark.gpu

TILE = "128x128w4"                                # the tile the sweep kept; forced by name its class stays gemm_f32h_128x128
GEOM = BM, BN, WGM, WGN = gc.FAMILIES["f32h"][2][TILE]
TM = BM // WGM
SK_TAG = "f32h_sk"                                # the automatic route's class: gemm_f32h_sk_128x128
KS = (128, 160, 512)
# feature set -> (FEATURES entry, scale unit).  Units: 99 puts a unit boundary inside the row tile (two running maxima per
# wavefront), TM = one unit per wavefront tile, 24 < TM splits every wavefront tile at odd rows (one tracker update per row).
FEATS = {"plain": (dict(), 99), "bias_gelu": (dict(act=1), TM), "residual_stats": (dict(R=True, stats=True), 99),
         "tracker_split": (dict(), 24)}


def _family(monkeypatch, tag):
    """run_case builds the class it expects from the family's profiler tag"""
    prec, _, tiles = gc.FAMILIES["f32h"]
    monkeypatch.setitem(gc.FAMILIES, "f32h", (prec, tag, tiles))


@pytest.mark.parametrize("feat", list(FEATS))
@pytest.mark.parametrize("M", [1, BM - 1, BM + 17])
def test_forced_wide_tile_at_its_edges(built_lib, gpu, monkeypatch, M, feat):
    from diarizen_amd import _lib
    f, unit = FEATS[feat]
    monkeypatch.setitem(gc.FEATURES, "FX", f)
    setter = _lib.load().dzn_op_set_gemm_cfg
    setter(TILE.encode())
    try:
        for N, odd in ((BN + 4, False), (2 * BN - 12, False), (2 * BN - 13, True)):
            for K in KS:
                gt.run_twice(gpu, "f32h", TILE, M, N, K, "FX", unit, odd=odd)
    finally:
        setter(b"auto")


@pytest.mark.parametrize("M", [1, 129])
@pytest.mark.parametrize("N,K,tag,geom", [(1024, 128, SK_TAG, GEOM), (1024, 512, SK_TAG, GEOM), (1024, 544, "f32h", (128, 128, 4, 1)),
                                          (448, 256, "f32h", (128, 64, 4, 1))])
def test_automatic_dispatch_by_n_and_k_alone(built_lib, gpu, monkeypatch, M, N, K, tag, geom):
    """run_case asserts the profiler class gemm_<tag>_<BM>x<BN> of the one launch, then its five checks"""
    _family(monkeypatch, tag)
    monkeypatch.setitem(gc.FEATURES, "FRS", dict(R=True, stats=True))
    gt.run_twice(gpu, "f32h", None, M, N, K, "FRS", 99, geom=geom)


def _launch(gpu, inp, rows, N, K, unit):
    """residual + statistics launch of the first `rows` rows of `inp` under the automatic rule -> (C, partial buffer, stats)"""
    from diarizen_amd import ops
    A, R = inp["A"][0][:rows].contiguous().to(gpu), inp["R"][0][:rows].contiguous().to(gpu)
    nu = gc.n_units(rows, unit)
    part = torch.full((rows, 32, 2), float("nan"), device=gpu)
    stats = torch.full((rows, 2), float("nan"), device=gpu)
    C = ops.gemm(A, inp["W"].to(gpu), bias=inp["bias"].to(gpu), R=R, precision=3, a_amax=inp["a_amax"][:nu].to(gpu),
                 amax_unit=unit, want_row_stats=True, stat_bufs=(part, stats))[0]
    torch.cuda.synchronize()
    return C.cpu(), part.cpu(), stats.cpu()


@pytest.fixture(scope="module")
def launches(built_lib, gpu):
    """N = 1024, K = 256, scale units of 43 rows (129 = 3 units): the M = 1000 launch, the M = 129 launch of its first rows, and
    the partial count the launcher reports after each"""
    from diarizen_amd import _lib
    M, N, K, unit = 1000, 1024, 256, 43
    inp = gc.make_inputs(M, N, K, unit)
    last = getattr(_lib.load(), "_Z23gemm_stat_partials_lastv")           # int gemm_stat_partials_last() (common.h)
    last.restype, last.argtypes = ctypes.c_int, []
    big = _launch(gpu, inp, M, N, K, unit)
    p_big = last()
    small = _launch(gpu, inp, 129, N, K, unit)
    return dict(inp=inp, big=big, small=small, P=(p_big, last()), N=N)


def test_rows_do_not_depend_on_the_batch(launches):
    (C, _, st), (c, _, s) = launches["big"], launches["small"]
    assert torch.isfinite(c).all() and torch.isfinite(s).all()
    assert torch.equal(am._bits(C[:129]), am._bits(c)), "C rows differ between the M = 1000 and the M = 129 launch"
    assert torch.equal(am._bits(st[:129]), am._bits(s)), "(mean, rstd) differ between the M = 1000 and the M = 129 launch"


def test_eight_partials_per_row_feed_gate_heads(launches, gpu):
    from diarizen_amd import ops
    assert launches["P"] == (8, 8)
    C, part, st = launches["big"]
    rows, N = C.shape
    flat = part.reshape(-1)
    assert torch.isfinite(flat[:rows * 16]).all() and torch.isnan(flat[rows * 16:]).all()       # [rows, 8, 2], nothing behind it
    partial = flat[:rows * 16].view(rows, 8, 2).contiguous().to(gpu)
    assert torch.equal(am._bits(ops.stats_finalize(partial, N).cpu()), am._bits(st))
    Htot = N // 64
    _, gamma, beta, Wg, bg, cst = am._gate_inputs(rows, Htot, False, True)
    x = C.to(gpu)
    dvecs = [t.to(gpu) for t in (gamma, beta, Wg, bg, cst)]
    hidx = torch.arange(Htot, dtype=torch.int32, device=gpu)
    gate_h, st_h = ops.gate_heads(x, *dvecs, hidx, partial)
    gate_s, _ = ops.gate_stats(x, *dvecs)
    torch.cuda.synchronize()
    assert torch.equal(am._bits(st_h.cpu()), am._bits(st))
    ref, bound, _, _ = es._reference(C, gamma, beta, Wg, bg, cst, 8)
    problems = []
    r = am._check_gate("gate_heads on the launch's partials", gate_h.cpu(), ref, bound, problems)
    # gate_stats' own bound on the same rows (test_attention_matrix_gpu.py's gate_stats case, restated)
    xd = C.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + es.EPS)
    e_mean = 23 * am.U * xd.abs().mean(1, keepdim=True)
    dv = xd - mean
    e_r = 0.5 * (2 * e_mean * rstd + 27 * am.U) + 3 * am.U
    yn = dv * rstd * gamma.double()
    y = yn + beta.double()
    ey = (rstd * gamma.double().abs()) * (e_mean + am.U * dv.abs()) + yn.abs() * (e_r + 2 * am.U) + am.U * y.abs()
    ref_s, bound_s, _ = am._gate_ref(y.view(rows, Htot, 64), ey.view(rows, Htot, 64), Wg, bg, cst, 16)
    am._check_gate("gate_stats on the stored rows", gate_s.cpu(), ref_s, bound_s, problems)
    d = float(((gate_h.cpu().double() - gate_s.cpu().double()).abs() / (bound + bound_s)).max())
    print(f"[short-K wide] gate_heads error / bound {r:.3f}; |gate_heads - gate_stats| / (sum of bounds) {d:.3f}")
    assert d <= 1.0 and not problems, "\n".join(problems + [f"gate_heads - gate_stats: {d:.3f} of the summed bounds"])
