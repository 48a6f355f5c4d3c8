"""CPU: the bounds of tests/_frontend_cases.py are neither loose nor tight by accident.  An IDEAL fp32 kernel (every operation
rounded once, in numpy float32; for conv01 the two-term fp16 operands and fp32 accumulation of the device kernel) under forward
order and the kernel's own order stays inside every bound with a QUARTER of its accumulation share on every case, each subtly
wrong kernel of the lists leaves the bound on at least one case, the lnq factor the built library ships holds its checks, and
the case tables reach what they claim.  The same references and bounds then judge the device in test_frontend_kernels_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest

import _frontend_cases as fc
from _frontend_cases import F32, F64, worst_ratio

P_HOST = 2                      # workgroups of the persistent-loop cases on the CPU (the device test reads the real count)


def _ideal(name, cases, inputs, run, bound, orders):
    worst = 0.0
    for c in cases:
        inp = inputs(c)
        ref, bnd = run(c, inp)["out"], bound(c, inp, 0.25)["out"]
        for oname, kw in orders.items():
            r = worst_ratio(run(c, inp, F32, **kw)["out"], ref, bnd)
            assert r <= 1.0, f"ideal fp32 kernel ({oname} order) at {r:.3f} of the bound with a quarter of its accumulation share: {c}"
            worst = max(worst, r)
    print(f"\n[front-end matrix] {name}: ideal / (bound at s = 1/4) = {worst:.3f}")


def _mutants(name, cases, inputs, run, bound, mutants):
    where = {}
    for c in cases:
        left = [m for m in mutants if m not in where]
        if not left:
            break
        inp = inputs(c)
        ref, bnd = run(c, inp)["out"], bound(c, inp)["out"]
        for m in left:
            r = worst_ratio(run(c, inp, mutant=m)["out"], ref, bnd)
            if r > 1.0:
                where[m] = (c["i"], r)
    print(f"\n[front-end matrix] {name}: mutants caught (case, error / bound): " + ", ".join(f"{m} ({i}, {r:.3g})" for m, (i, r) in where.items()))
    assert set(where) == set(mutants), f"no case of the table holds these wrong kernels outside the bound: {sorted(set(mutants) - set(where))}"


def test_lnq_reference_and_library(built_lib):
    from diarizen_amd import ops
    from diarizen_amd._lib import DznError
    for c in fc.LNQ_CASES:
        inp = fc.lnq_inputs(c)
        fc.lnq_check(c, inp, fc.lnq_run(c, inp)["lnq"].astype(F32))
        got = ops.conv0_lnq(inp["w"], c["C0"], c["k"])
        fc.lnq_check(c, inp, got)
        assert np.array_equal(got.view(np.uint32), ops.conv0_lnq(inp["w"], c["C0"], c["k"]).view(np.uint32))
    w = fc.lnq_inputs(fc.LNQ_CASES[0])["w"]
    for C0, k in ((0, 10), (4, 0), (4, 11)):
        with pytest.raises(DznError):
            ops.conv0_lnq(w, C0, k)


def test_conv0():
    orders = dict(forward=dict(ssum=fc.seq_sum), kernel=dict(ssum=fc.phase_sum(64)))
    _ideal("conv0", fc.c0_cases(), fc.c0_inputs, fc.c0_run, fc.c0_bound, orders)
    _mutants("conv0", fc.c0_cases(), fc.c0_inputs, fc.c0_run, fc.c0_bound, fc.C0_MUTANTS)


def test_conv0_product_form_fails_on_the_stress_case():
    """var as the plain fp32 sum x^T Q x, on DC-blocking taps and a slow sine: the printed ratio is how far outside the bound it
    lands (3.5), while the ideal kernel of the factor form stays inside it (test_conv0)"""
    c = next(c for c in fc.c0_cases() if c["stress"] and c["mode"] == "lnq")
    inp = fc.c0_inputs(c)
    r = worst_ratio(fc.c0_run(c, inp, mutant="var_product_form")["out"], fc.c0_run(c, inp)["out"], fc.c0_bound(c, inp)["out"])
    print(f"\n[front-end matrix] conv0 stress case: var_product_form error / bound = {r:.3g}")
    assert r > 1.0


def test_conv01():
    cases = fc.c01_cases(P_HOST)
    orders = dict(forward=dict(ssum=fc.seq_sum), kernel=dict(ssum=fc.phase_sum(2), kernel_order=True))
    _ideal("conv01", cases, fc.c01_inputs, fc.c01_run, fc.c01_bound, orders)
    # the persistent-loop cases first: they are the only ones where a workgroup has a previous item
    _mutants("conv01", cases[-3:] + cases[:-3], fc.c01_inputs, fc.c01_run, fc.c01_bound, fc.C01_MUTANTS)


def test_frag_reindex_and_split_statement():
    assert sorted(fc.H2_POS) == list(range(32)) and fc.H2_POS[:6] == [0, 1, 2, 3, 8, 9] and fc.H2_POS[16] == 4
    for rows, K in fc.FRAG_SHAPES:
        W = fc.frag_inputs(rows, K)
        planes, inv = fc.h2_split(W)
        assert inv[rows // 2] == 1.0 and not planes[rows // 2].any()
        m = np.abs(W[rows - 1]).max()
        assert m == 1.0 and inv[rows - 1] == 2.0 ** -14
        fr = fc.frag_reindex(planes)
        assert fr.shape == (K // 32, rows // 16, 2, 16, 32)
        r, k = rows - 3, K - 5
        assert fr[k // 32, r // 16, 1, r % 16, k % 32] == planes[r, k // 32, 1, k % 32]
        hi = planes[:, :, 0].reshape(rows, K).view(np.float16).astype(F64)
        lo = planes[:, :, 1].reshape(rows, K).view(np.float16).astype(F64)
        assert (np.abs((hi + lo) * inv[:, None] - W) <= 2.0 ** -21 * np.abs(W) + 2.0 ** -38 * np.abs(W).max(1, keepdims=True)).all()


def test_tables_reach_what_they_claim():
    c0 = fc.c0_cases()
    assert {fc.c0_cpl(c["C0"], c["Cp"]) for c in c0} == {4, 8}
    for cpl in (4, 8):
        sub = [c for c in c0 if fc.c0_cpl(c["C0"], c["Cp"]) == cpl]
        assert {c["mode"] for c in sub} == set(fc.MODES)
        assert {c["T0"] for c in sub} >= set(fc.T0S)
    assert {(c["C0"], c["Cp"]) for c in c0} == set(fc.WIDTHS) and {(c["k"], c["s"]) for c in c0} == set(fc.KS)
    assert {c["stats"] for c in c0} == {True, False} and len(c0) <= 48
    assert any(c["T0"] < 64 for c in c0) and any(c["T0"] > 64 for c in c0)
    assert any((c["k"], c["s"]) == (10, 8) and c["T0"] >= 64 for c in c0)          # the largest LDS stage: 63 * 8 + 10 samples
    assert all((c["T0"] - 1) * c["s"] + c["k"] <= c["N"] <= (c["T0"] - 1) * c["s"] + c["k"] + 4 for c in c0)
    for P in (P_HOST, 256):
        c01 = fc.c01_cases(P)
        assert {c["T0"] - 2 * c["T1"] for c in c01} == {1, 2}
        assert {-(-c["T1"] // fc.TILE) for c in c01} == {1, 2, 3}
        assert {c["C1"] for c in c01} >= {81, 160} and {c["C0"] for c in c01} == {128, 192, 512}
        assert {c["T1"] for c in c01} >= set(fc.C01_T1)
        assert {(c["ln"], c["amax"]) for c in c01} >= {(True, "zero"), (True, "high"), (True, "none"), (False, "none")}
        assert {c["wstats"] for c in c01} == {True, False}
        assert all(c["T1"] <= (c["T0"] - 3) // 2 + 1 and (c["T0"] - 1) * 5 + 10 <= c["N"] for c in c01)
        assert [(c["B"], c["T1"]) for c in c01[-3:]] == [(2 * P + 1, 3), (P + 1, 128), (P + 1, 128)]
        assert all(c["B"] * -(-c["T1"] // fc.TILE) <= 256 for c in c01[:-3])        # one item per workgroup everywhere else
