"""CPU: the bounds of tests/_small_cases.py are neither loose nor tight by accident.  For every kernel an IDEAL fp32 kernel (every
operation rounded once, in numpy float32) under two accumulation orders — forward, and the kernel's own phases / chunks — stays
inside the bound with a QUARTER of its accumulation share (single roundings at face value) on every case of the table, and each subtly wrong kernel of the list below exceeds the bound on at
least one case.  The same references and bounds then judge the device kernels in test_small_kernels_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _small_cases as sc
from _small_cases import F32, worst_ratio


def _ideal(cases, inputs, run, bound, orders, keys):
    worst = 0.0
    for c in cases:
        inp = inputs(c)
        ref, bnd = run(c, inp), bound(c, inp, 0.25)
        for name, ssum in orders(c).items():
            got = run(c, inp, F32, ssum)
            for k in keys:
                r = worst_ratio(got[k], ref[k], bnd[k])
                assert r <= 1.0, f"ideal fp32 kernel ({name} order) at {r:.3f} of the bound of {k} with a quarter of its accumulation share: {c}"
                worst = max(worst, r)
    print(f"ideal / (bound at s = 1/4): {worst:.3f}")


def _mutants(cases, inputs, run, bound, mutants, keys, **kw):
    left = set(mutants)
    for c in cases:
        if not left:
            break
        inp = inputs(c)
        ref, bnd = run(c, inp), bound(c, inp)
        for m in sorted(left):
            got = run(c, inp, mutant=m, **kw)
            if any(worst_ratio(got[k], ref[k], bnd[k]) > 1.0 for k in keys):
                left.discard(m)
    assert not left, f"no case of the table holds these wrong kernels outside the bound: {sorted(left)}"


def test_glu_dwconv():
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.rev_sum)      # the kernel's taps run forward: the other order is backward
    _ideal(sc.dw_cases(), sc.dw_inputs, sc.dw_run, sc.dw_bound, orders, ["out"])
    _mutants(sc.dw_cases(), sc.dw_inputs, sc.dw_run, sc.dw_bound, ["halo_neighbour", "tap_shift"], ["out"])


def test_halo_mutant_is_seen_in_the_quiet_windows():
    """the loud window 1 is what makes a halo read from a neighbour visible: windows 0 and 2 alone exceed their bound"""
    c = next(c for c in sc.dw_cases() if c["L"] == 5 and c["ks"] == 31)
    inp = sc.dw_inputs(c)
    ref, bnd, got = sc.dw_run(c, inp)["out"], sc.dw_bound(c, inp)["out"], sc.dw_run(c, inp, mutant="halo_neighbour")["out"]
    assert worst_ratio(got[[0, 2]], ref[[0, 2]], bnd[[0, 2]]) > 1e3


def test_classify():
    cases = sc.cls_cases()
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.phase_sum(64))
    _ideal(cases, sc.cls_inputs, sc.cls_run, sc.cls_bound, orders, ["logp", "soft"])
    _mutants(cases, sc.cls_inputs, sc.cls_run, sc.cls_bound, ["soft_extra"], ["soft"])
    tie_seen = False
    for c in cases:
        inp = sc.cls_inputs(c)
        ref, bnd = sc.cls_run(c, inp), sc.cls_bound(c, inp)
        n_un = int(bnd["unresolved"].sum())
        assert n_un <= 0.01 * c["rows"], f"{n_un} of {c['rows']} rows left out: {c}"
        keep = ~bnd["unresolved"]
        assert np.array_equal(sc.cls_run(c, inp, F32, sc.phase_sum(64))["multilabel"][keep], ref["multilabel"][keep])
        last = sc.cls_run(c, inp, mutant="last_tie")
        tie_seen |= not np.array_equal(last["multilabel"][keep], ref["multilabel"][keep])
    assert tie_seen, "no kept row of any case tells the first maximum from the last"


def test_powerset_mapping_is_the_reference_order():
    assert sc.powerset_mapping(3, 2).tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]]
    for (NC, S), k in sc.POWERSETS.items():
        assert sc.powerset_mapping(S, k).shape == (NC, S)


def test_groupnorm_gelu():
    cases = sc.gn_cases()
    for name in ("forward", "kernel"):
        def run(c, inp, dt=sc.F64, ssum=sc.exact_sum, mutant=None):
            return sc.gn_run(c, inp, dt, ssum, mutant, chunked=(name == "kernel" and dt is F32))
        orders = lambda c: {name: sc.seq_sum if name == "forward" else sc.phase_sum(sc.gn_nph(c))}
        _ideal(cases, sc.gn_inputs, run, sc.gn_bound, orders, ["y"])
    _mutants(cases, sc.gn_inputs, sc.gn_run, sc.gn_bound, ["last_chunk_128", "no_cross"], ["y"])


def test_layernorm():
    cases = sc.ln_cases()
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.phase_sum(64))
    _ideal(cases, sc.ln_inputs, sc.ln_run, sc.ln_bound, orders, ["y"])
    _mutants(cases, sc.ln_inputs, sc.ln_run, sc.ln_bound, ["div_cpad"], ["y"])


def test_layernorm_cases_reach_every_instantiation_and_both_loops():
    hit = {sc.ln_dispatch(c["C"], c["Cpad"]) for c in sc.ln_cases() if c["path"] == "v4"}
    assert hit == sc.LN_TABLE
    for pair, gnv in sc.LN_V4.items():
        assert sc.ln_dispatch(*pair) == gnv
    for pair in sc.LN_WIDE:
        assert sc.ln_dispatch(*pair) is None
    assert sc.ln_iters(*sc.LN_ITERS) > 1
    for path in ("v4", "offset", "wide"):
        assert {c["rows"] for c in sc.ln_cases() if c["path"] == path} >= {1, 3, 5, 77}
    for key, values in (("affine", {"gb", "none", "g", "b"}), ("post", {True, False}), ("gelu", {True, False}), ("inplace", {True, False}),
                        ("amax_unit", {None, 0, 1, 7})):
        for path in ("v4", "offset", "wide"):
            assert {c[key] for c in sc.ln_cases() if c["path"] == path} == values, (key, path)


def test_wave_stats():
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.phase_sum(1024))
    _ideal(sc.WS_N, sc.wv_inputs, sc.wv_run, sc.wv_bound, orders, ["stats"])


def test_ws_sum_emulation_is_inside_the_bound():
    g = np.random.default_rng(5)
    for k in sc.WSUM_COUNTS:
        xs, ws = [g.standard_normal(1020).astype(F32) for _ in range(k)], sc.wsum_weights(k)
        assert worst_ratio(sc.wsum_run(xs, ws, F32), sc.wsum_run(xs, ws), sc.wsum_bound(xs, ws, 0.25)) <= 1.0


def test_frame_prep():
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.phase_sum(64))
    _ideal(sc.fp_cases(), sc.fp_inputs, sc.fp_run, sc.fp_bound, orders, ["frames"])
    _mutants(sc.fp_cases(), sc.fp_inputs, sc.fp_run, sc.fp_bound, ["first_zero", "early64"], ["frames"])


def test_power_and_log_cmn():
    _ideal(sc.mel_cases(), sc.pw_inputs, sc.pw_run, sc.pw_bound, lambda c: dict(forward=None), ["pw"])
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.phase_sum(16))
    _ideal(sc.mel_cases(), sc.cmn_inputs, sc.cmn_run, sc.cmn_bound, orders, ["mel"])
    _mutants(sc.mel_cases(), sc.cmn_inputs, sc.cmn_run, sc.cmn_bound, ["mean16"], ["mel"])


def test_stem_conv():
    cases = [dict(NB=NB, T=T) for NB, T in sc.STEM]
    run = lambda c, inp, *a, **k: sc.stem_run(c["NB"], c["T"], inp, *a, **k)
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.rev_sum)
    _ideal(cases, lambda c: sc.stem_inputs(c["NB"], c["T"]), run, lambda c, inp, s=1.0: sc.stem_bound(c["NB"], c["T"], inp, s), orders, ["img"])


def test_stats_pool():
    cases = sc.pool_cases()
    orders = lambda c: dict(forward=sc.seq_sum, kernel=sc.rev_sum)      # the kernel's frames run forward: the other order is backward
    _ideal(cases, sc.pool_inputs, sc.pool_run, sc.pool_bound, orders, ["stats"])
    _mutants(cases, sc.pool_inputs, sc.pool_run, sc.pool_bound, ["round", "no_eps", "div_v1"], ["stats"])


def test_stats_pool_index_is_torch_nearest():
    cross = 0
    for c in sc.pool_cases():
        W, L = c["W"], c["L"]
        want = torch.nn.functional.interpolate(torch.arange(L, dtype=torch.float32)[None, None], size=W, mode="nearest")[0, 0]
        assert sc.pool_src(W, L).tolist() == want.long().tolist(), (W, L)
        cross += int((sc.pool_src(W, L) != np.minimum(np.floor(np.arange(W) * (L / W)), L - 1)).sum())
    print(f"frames whose float32 index differs from the float64 one: {cross}")


def test_compact_reference_flags():
    for B in sc.ACTIVE_B:
        assert sc.active_flags(B, "third").sum() == -(-B // 3) and sc.active_flags(B, "none").sum() == 0
