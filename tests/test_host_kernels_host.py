"""CPU: the references, bounds and case tables of tests/_host_cases.py are neither loose nor blind.  For every family of the
host-stage matrix an IDEAL kernel (float64, every operation rounded once, forward order and the kernel's own order) stays inside the
bound with a QUARTER of its accumulation share, scipy's dendrogram ids are stable on every linkage case, the corrected numpy model
of prepare_masks equals scipy on every case, and each subtly wrong kernel of the lists below is caught by at least one case.  The
same references, bounds and checks then judge the device kernels in test_host_kernels_gpu.py."""
from __future__ import annotations

import math

import numpy as np

import _host_cases as hc
from _host_cases import F64, LD, U, worst_ratio


def _axis_twice(cases, axes):
    for key, values in axes.items():
        for v in values:
            assert sum(1 for c in cases if c[key] == v) >= 2, f"{key} = {v} appears less than twice"


# ---- linkage --------------------------------------------------------------------------------------------------------------
def test_linkage_table_covers_every_axis_value_twice():
    cases = hc.lk_cases()
    assert 24 <= len(cases) <= 30
    _axis_twice(cases, dict(n=hc.LK_N, dim=hc.LK_DIM, scale=hc.LK_SCALE))


def test_linkage_reference_is_stable_and_the_model_reproduces_it():
    """scipy's ids do not move under relative 1e-12 noise on the condensed distances (no case is excluded: an unstable one gets
    another seed in LK_SEED), and the numpy model of pdist_kernel leads to scipy's dendrogram and stays inside both bounds"""
    worst = [0.0, 0.0]
    for c in hc.lk_cases():
        inp = hc.lk_inputs(c)
        assert hc.lk_stable(c, inp), f"scipy's dendrogram ids move under 1e-12 noise: {c}"
        ref = hc.lk_ref(c, inp)
        r = hc.lk_check(c, ref, hc.lk_model_Z(c, inp))
        assert max(r) < 1.0, f"the model of pdist_kernel at {r} of (tolerance, singleton bound): {c}"
        worst = [max(a, b) for a, b in zip(worst, r)]
        if c["n"] <= 65:
            D = hc.lk_pdist_model(inp["e"])
            assert hc.lk_same_ids(hc.lk_naive(D), ref["Z"]), f"the full-matrix greedy model differs from scipy: {c}"
    print(f"pdist model: height / tolerance {worst[0]:.3g}, singleton merges / bound {worst[1]:.3f}")


def test_linkage_structural_cases_are_what_they_claim():
    by = {c["kind"]: c for c in hc.lk_cases()}
    Z = hc.lk_ref(by["inversions"], hc.lk_inputs(by["inversions"]))["Z"]
    assert (np.diff(Z[:, 2]) < 0).any(), "no inversion in scipy's dendrogram"
    c = by["triplets"]
    ref = hc.lk_ref(c, hc.lk_inputs(c))
    Z, n = ref["Z"], c["n"]
    # a triplet: two singletons merge, then the third singleton joins that very cluster -> its two nearest were both retired
    joined = sum(1 for k, row in enumerate(Z) if row[3] == 3 and min(row[0], row[1]) < n and max(row[0], row[1]) >= n
                 and ref["single"][int(max(row[0], row[1])) - n])
    assert joined >= 30, joined


def test_linkage_mutants_change_the_ids():
    left = {"k_tail", "j_tile", "diag_zero"}
    for c in hc.lk_cases():
        if not left:
            break
        inp = hc.lk_inputs(c)
        ref = hc.lk_ref(c, inp)["Z"]
        for m in sorted(left):
            if m == "diag_zero" and c["n"] > 65:
                continue
            if not hc.lk_same_ids(hc.lk_model_Z(c, inp, m), ref):
                left.discard(m)
    assert not left, f"no case of the table tells these wrong pdist kernels from the right one: {sorted(left)}"


# ---- cdist_cosine ---------------------------------------------------------------------------------------------------------
def test_cdist_table_and_inputs():
    cases = hc.cd_cases()
    _axis_twice(cases, dict(n=(1, 255, 256, 257), k=(1, 2, 13, 33), dim=(1, 3, 64, 255, 256, 257)))
    assert any((c["n"] * c["k"]) % 256 and 256 % c["k"] for c in cases)
    over = 0
    for c in cases:
        inp = hc.cd_inputs(c)
        r = hc.cd_run(c, inp)
        with np.errstate(invalid="ignore"):
            over += int((np.abs(r["pre"]) > 1.0).sum())
        if c["n"] > 1:
            assert np.isnan(r["out"][5]).all() and np.isnan(r["out"][6]).all()
            assert (c["k"] == 1 or np.isnan(r["out"][:, 1]).all()) and np.isfinite(r["out"][7:100, 0]).all()
    assert over > 0, "no case reaches |cos| > 1 before the clip: the clip is untested"
    print(f"elements with |cos| > 1 before the clip: {over}")


def test_cdist_in_order_emulation_against_longdouble():
    worst = 0.0
    for c in hc.cd_cases():
        inp = hc.cd_inputs(c)
        pre, ex = hc.cd_run(c, inp)["pre"], hc.cd_exact(c, inp)
        ok = np.isfinite(pre)
        assert np.array_equal(ok, np.isfinite(ex["pre"].astype(F64)))
        ref = ex["pre"][ok]
        bnd = 0.25 * (c["dim"] + 8) * U * ex["sabs"][ok] + 8 * U * np.abs(ref.astype(F64))
        err = np.abs(pre[ok].astype(LD) - ref).astype(F64)
        r = float((err / bnd).max()) if err.size else 0.0
        assert r <= 1.0, f"in-order emulation at {r:.3f} of the bound at s = 1/4: {c}"
        worst = max(worst, r)
        got = hc.cd_run(c, inp, hc.phase_sum(4))["out"]                 # another order of the same sums: the bound of the device test is
        assert hc.cd_check(c, inp, got) < math.inf                     # about sqrt and division only, the exact properties hold anyway
    print(f"in-order emulation / (bound at s = 1/4): {worst:.3f}")


def test_cdist_mutants():
    left = {"no_clip", "norm_f32", "row_mod_n"}
    for c in hc.cd_cases():
        inp = hc.cd_inputs(c)
        ref, bnd = hc.cd_run(c, inp)["out"], hc.cd_bound(c, inp)["out"]
        assert hc.cd_check(c, inp, ref, ref, bnd) == 0.0
        for m in sorted(left):
            if hc.cd_check(c, inp, hc.cd_run(c, inp, mutant=m)["out"], ref, bnd) > 1.0:
                left.discard(m)
    assert not left, f"no case of the table catches these wrong kernels: {sorted(left)}"


# ---- vbx ------------------------------------------------------------------------------------------------------------------
def test_vbx_table_covers_every_axis_value_twice():
    cases = hc.vb_cases()
    _axis_twice(cases, dict(E=hc.VB_E, K=hc.VB_K, D=hc.VB_D))
    assert any(c["D"] >= 256 and c["K"] >= 9 and c["E"] > 256 for c in cases)
    assert any(c["sat"] for c in cases) and any(c["pi0"] for c in cases)


def test_vbx_ideal_kernel_and_mutants():
    left = {"ns_col", "last_chunk_256", "tile0", "lane_tail", "no_shift"}
    worst, nonfinite, nsat = 0.0, False, 0
    for c in hc.vb_cases():
        inp = hc.vb_inputs(c)
        ref, bq, bnd = hc.vb_run(c, inp), hc.vb_bound(c, inp, 0.25), hc.vb_bound(c, inp)
        if c["sat"]:
            assert bnd["sat"][0] and bnd["sat"][c["E"] // 2], f"the scaled rows do not lead by more than 745: {c}"
            g = ref["gamma"][bnd["sat"]].astype(F64)
            assert np.isin(g, (0.0, 1.0)).all()
            nsat += int(bnd["sat"].sum())
        if c["pi0"]:
            assert inp["lpi"][-1] == math.log(1e-8)
        for order in ("forward", "kernel"):
            r = hc.vb_check(c, ref, bq, hc.vb_run(c, inp, F64, order))
            assert r <= 1.0, f"ideal float64 kernel ({order} order) at {r:.3f} of the bound with a quarter of its accumulation share: {c}"
            worst = max(worst, r)
        for m in sorted(left):
            got = hc.vb_run(c, inp, F64, "kernel", m)
            if m == "no_shift":
                if c["sat"] and not np.isfinite(got["gamma"]).all():
                    nonfinite = True
                    left.discard(m)
            elif hc.vb_check(c, ref, bnd, got) > 1.0:
                left.discard(m)
    assert not left, f"no case of the table catches these wrong kernels: {sorted(left)}"
    assert nonfinite and nsat > 0
    print(f"ideal / (bound at s = 1/4): {worst:.3f}; saturated rows: {nsat}")


# ---- prepare_masks --------------------------------------------------------------------------------------------------------
def test_prepare_masks_table():
    cases = hc.pm_cases()
    assert 36 <= len(cases) <= 44
    _axis_twice(cases, dict(L=hc.PM_L, S=hc.PM_S, median=hc.PM_MEDIAN, exclude_overlap=(0, 1), B=(1, 3)))
    assert {c["min_num_frames"] for c in cases} >= {0, 1} and any(c["min_num_frames"] == c["L"] > 1 for c in cases)
    assert sum(1 for c in cases if (c["L"] * c["S"]) % 4) >= 5 and sum(1 for c in cases if not c["want_masks"]) == 1
    lds = lambda L, S: 2 * ((L * S + 3) & ~3) + 32
    assert lds(*hc.PM_LDS_OK) <= 65536 < lds(*hc.PM_LDS_REFUSED)


def test_prepare_masks_model_equals_scipy_and_the_old_rule_does_not():
    caught = []
    for c in hc.pm_cases() + [dict(i=99, B=1, L=hc.PM_LDS_OK[0], S=hc.PM_LDS_OK[1], median=21, exclude_overlap=1, min_num_frames=2, want_masks=True)]:
        inp = hc.pm_inputs(c)
        ref, got, old = hc.pm_ref(c, inp), hc.pm_run(c, inp), hc.pm_run(c, inp, "reflect_once")
        assert np.array_equal(got["filtered"], ref["filtered"]) and np.array_equal(got["masks"], ref["masks"]), c
        if not np.array_equal(old["filtered"], ref["filtered"]):
            caught.append((c["L"], c["median"]))
    assert caught and all(L < m // 2 + 1 for L, m in caught), caught
    assert any(m == 11 for _, m in caught) and any(m == 21 for _, m in caught)
    print(f"(L, median) at which one reflection and a clamp is not scipy's reflect: {sorted(set(caught))}")


# ---- speaker_count / cluster_activations ----------------------------------------------------------------------------------
def test_aggregation_table_and_mutants():
    cases = [c for c in hc.ag_cases() if c["kind"] != "stride"]
    _axis_twice(cases, dict(C=hc.AG_C, L=hc.AG_L, S=hc.AG_S, K=hc.AG_K))
    assert hc.AG_STRIDE["C"] * hc.AG_STRIDE["L"] > 8192 * 256
    left = {"floor_half", "sum", "past_T", "label_K"}
    labels, uncovered = set(), 0
    for c in cases:
        inp = hc.ag_inputs(c)
        ref = hc.ag_run(c, inp)
        labels |= set(np.unique(inp["hard"][:c["C"]]).tolist()) & {-2, -1} | ({"K"} if (inp["hard"][:c["C"]] == c["K"]).any() else set())
        if c["C"] and c["kind"] == "random":
            assert inp["start"].min() < 0 and (c["C"] < 2 or inp["start"].max() + c["L"] > inp["T"])
            cover = np.zeros(inp["T"] + 2 * c["L"] + 1, bool)
            for s in inp["start"]:
                cover[s + c["L"]:s + 2 * c["L"]] = True
            uncovered += int((~cover[c["L"]:c["L"] + inp["T"]]).sum())
        for m in sorted(left):
            got = hc.ag_run(c, inp, m)
            if not (np.array_equal(got["count"], ref["count"]) and np.array_equal(got["act"], ref["act"])):
                left.discard(m)
    assert not left, f"no case of the table catches these wrong kernels: {sorted(left)}"
    assert labels == {-2, -1, "K"} and uncovered > 0
    c = next(c for c in cases if c["kind"] == "halves")
    assert hc.ag_run(c, hc.ag_inputs(c))["count"].tolist() == [0, 2, 2, 1, 0, 0, 0]


def test_aggregation_reference_is_the_host_pipeline():
    """postprocess.speaker_count / reconstruct's arithmetic (float32 accumulators, np.rint) on a case they can express: starts
    inside [0, T - L]"""
    g = np.random.default_rng(3)
    C, L, S, K, T = 6, 9, 3, 4, 40
    c = dict(C=C, L=L, S=S, K=K)
    inp = dict(seg=(g.random((C, L, S)) < 0.5).astype(np.uint8), start=np.sort(g.integers(0, T - L, C)).astype(np.int32),
               hard=g.integers(-2, K, (C, S)).astype(np.int8), T=T)
    out, cnt = np.zeros(T, np.float32), np.zeros(T, np.float32)
    for w in range(C):
        s0 = inp["start"][w]
        out[s0:s0 + L] += inp["seg"][w].sum(1).astype(np.float32)
        cnt[s0:s0 + L] += 1
    want = np.rint(np.where(cnt > 0, out / np.maximum(cnt, 1e-12), 0)).astype(np.uint8)
    assert np.array_equal(hc.ag_run(c, inp)["count"], want)


# ---- hysteresis -----------------------------------------------------------------------------------------------------------
def test_hysteresis_cases_and_mutant():
    cases = hc.hy_cases()
    assert {c["n"] for c in cases} == set(hc.HY_N) and {(c["onset"], c["offset"]) for c in cases} == set(hc.HY_THR)
    caught = False
    for c in cases:
        inp = hc.hy_inputs(c)
        assert set(np.unique(inp["y"]).tolist()) <= {0.0, 0.5, 1.0}
        if c["n"] >= 1023:
            per = -(-c["n"] // hc.HY_THREADS)
            run = max(len(r) for r in "".join("u" if v == 0.5 else "d" for v in inp["y"]).split("d"))
            assert run > 5 * per, "no undecided run longer than several threads' chunks"
        ref = hc.hy_run(c, inp)["active"]
        assert len(ref) == c["n"] - c["t0"]
        if (c["onset"], c["offset"]) == (1.0, 0.0):
            assert (ref == (c["entry"] or 0)).all()                       # nothing but frame 0 / the entry state ever decides
        caught |= not np.array_equal(hc.hy_run(c, inp, "non_strict")["active"], ref)
    assert caught, "no case tells > from >= at score == threshold"
