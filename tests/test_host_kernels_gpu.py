"""The host-stage matrix (device): csrc/linkage.hip through ops.linkage_centroid and ops.cdist_cosine, csrc/vbx.hip one kernel at a
time through ops.VbxState, and the integer / byte kernels of csrc/post.hip (prepare_masks through Engine.prepare_masks,
count_accum / count_finalize / cluster_accum through the raw ABI as DevicePost calls it, hysteresis_kernel through
dzn_detect_range) against the references, bounds and exact properties of tests/_host_cases.py, at the shapes where these kernels
handle an edge by hand.  Each family prints its worst error / bound ratio and records it in host_kernels.json under the directory that
DZN_TEST_RECORD_DIR names, when it names one.  test_host_kernels_host.py shows what the bounds let through and what they do not."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import _host_cases as hc
from _host_cases import F64
from diarizen_amd import _lib, ops
from diarizen_amd._lib import DznError

pytestmark = pytest.mark.gpu

_RECORD_DIR = os.environ.get("DZN_TEST_RECORD_DIR", "")


def _record(**kw):
    print("\n[host-kernel matrix] " + ", ".join(f"{k} = {v}" for k, v in kw.items()))
    if _RECORD_DIR and os.path.isdir(_RECORD_DIR):
        path = os.path.join(_RECORD_DIR, "host_kernels.json")
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.update(kw)
        with open(path, "w") as f:
            json.dump(old, f, indent=1)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- linkage + pdist ------------------------------------------------------------------------------------------------------
def test_linkage_and_pdist_at_the_tile_edges(built_lib, gpu):
    w_h, w_p, at = 0.0, 0.0, None
    for c in hc.lk_cases():
        inp = hc.lk_inputs(c)
        ref = hc.lk_ref(c, inp)
        Z = ops.linkage_centroid(inp["e"])
        assert hc.lk_same_ids(Z, ref["Z"]), f"ids / sizes differ from scipy's dendrogram: {c}"
        rh, rp = hc.lk_check(c, ref, Z)
        print(f"linkage {c}: height / tolerance {rh:.3g}, singleton merges / bound {rp:.3f}")
        if rp >= w_p:
            w_p, at = rp, c
        w_h = max(w_h, rh)
        assert np.array_equal(Z.view(np.uint64), ops.linkage_centroid(inp["e"]).view(np.uint64)), f"a second call differs: {c}"
    _record(linkage_height_over_tolerance=w_h, pdist_singleton_over_bound=w_p)
    assert w_h <= 1.0, f"merge heights at {w_h:.3g} of 1e-12 max(1, max height)"
    assert w_p < 1.0, f"singleton merges (pure pdist outputs) at {w_p:.3f} of (dim + 8 + 2) u at {at}"


def test_linkage_nan_row_is_refused_and_the_next_call_is_right(built_lib, gpu):
    """no pair left to merge (STEP_FAIL) -> DZN_E_INVALID; the arena and the stream are as good as before"""
    c = next(c for c in hc.lk_cases() if c["n"] == 65 and c["kind"] == "clustered")
    inp = hc.lk_inputs(c)
    bad = inp["e"].copy()
    bad[7] = np.nan
    with pytest.raises(DznError, match="invalid argument"):
        ops.linkage_centroid(bad)
    assert hc.lk_same_ids(ops.linkage_centroid(inp["e"]), hc.lk_ref(c, inp)["Z"])


# ---- cdist_cosine ---------------------------------------------------------------------------------------------------------
def test_cdist_cosine_against_its_own_statement(built_lib, gpu):
    worst, at, exact, total = 0.0, None, 0, 0
    for c in hc.cd_cases():
        inp = hc.cd_inputs(c)
        ref = hc.cd_run(c, inp)["out"]
        got = ops.cdist_cosine(inp["e"], inp["cent"])
        r = hc.cd_check(c, inp, got, ref)
        ok = ~np.isnan(ref)
        exact += int((got[ok] == ref[ok]).sum())
        total += int(ok.sum())
        print(f"cdist {c}: error / bound {r:.3f}")
        assert r < math.inf, f"NaN pattern, ties of identical rows or the range [0, 2]: {c}"
        if r >= worst:
            worst, at = r, c
    _record(cdist_over_bound=worst, cdist_bit_exact_fraction=exact / max(total, 1))
    assert worst < 1.0, f"cdist_cosine at {worst:.3f} of 8 u |cos| + u at {at}"


# ---- vbx ------------------------------------------------------------------------------------------------------------------
def test_vbx_kernels_one_at_a_time(built_lib, gpu):
    worst, at = 0.0, None
    for c in hc.vb_cases():
        inp = hc.vb_inputs(c)
        ref, bnd = hc.vb_run(c, inp), hc.vb_bound(c, inp)
        st = ops.VbxState(inp["X"], inp["Phi"], inp["g0"])
        try:
            got = dict(stats=st.stats())                                        # vb_setup (through rho), vb_accum, vb_reduce
            got["total"] = st.estep(inp["alpha"], inp["ck"], inp["lpi"], hc.VB_FA)
            got["gamma"] = st.gamma()
        finally:
            st.close()
        assert np.isfinite(got["gamma"]).all() and np.isfinite(got["total"]), f"non-finite responsibilities: {c}"
        r = hc.vb_check(c, ref, bnd, got)
        parts = [hc.worst_ratio(got[k], np.asarray(ref[k], F64), bnd[k]) for k in ("stats", "gamma", "total")]
        print(f"vbx {c}: stats {parts[0]:.3f}, gamma {parts[1]:.3f}, total {parts[2]:.3f} of their bounds")
        assert r < math.inf, f"a row led by more than 745 is not exactly 0 / 1: {c}"
        if r >= worst:
            worst, at = r, c
    _record(vbx_over_bound=worst)
    assert worst < 1.0, f"vbx at {worst:.3f} of its bound at {at}"


# ---- prepare_masks --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(built_lib, gpu):
    """the smallest engine per S: the kernel takes S from the handle and everything else from the tensor"""
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.engine import Engine
    from testkit.weights import seg_state_dict
    made = {}

    def get(S):
        if S not in made:           # segmentation only, as the detection pipelines build it
            cfg = replace(get_seg_config("tiny_ln"), max_speakers_per_chunk=S, max_speakers_per_frame=hc.PM_FRAME[S])
            made[S] = Engine(cfg, seg_state_dict(cfg, 0), None, None, max_batch=3, max_samples=16000, precision="f32", device=gpu)
        return made[S]
    yield get
    for e in made.values():
        e.close()


def _pm_check(engines, gpu, c):
    inp = hc.pm_inputs(c)
    ref = hc.pm_ref(c, inp)
    filt, masks = engines(c["S"]).prepare_masks(_dev(inp["raw"], gpu), c["median"], bool(c["exclude_overlap"]), c["min_num_frames"],
                                                want_masks=c["want_masks"])
    torch.cuda.synchronize()
    assert np.array_equal(filt.cpu().numpy(), ref["filtered"]), f"median filter differs from scipy's: {c}"
    if c["want_masks"]:
        assert np.array_equal(masks.cpu().numpy().view(np.uint32), ref["masks"].view(np.uint32)), f"masks differ: {c}"
    else:
        assert masks is None


def test_prepare_masks_equals_scipy_at_every_edge(engines, gpu):
    for c in hc.pm_cases():
        _pm_check(engines, gpu, c)


def test_prepare_masks_lds_limit(engines, gpu):
    """2 round4(L S) + 32 bytes of LDS: the largest window that fits runs and is right, the next is refused and writes nothing"""
    L, S = hc.PM_LDS_OK
    _pm_check(engines, gpu, dict(i=99, B=1, L=L, S=S, median=21, exclude_overlap=1, min_num_frames=2, want_masks=True))
    L, S = hc.PM_LDS_REFUSED
    eng = engines(S)
    raw = _dev(hc.pm_inputs(dict(i=98, B=1, L=L, S=S))["raw"], gpu)
    filt = torch.full((1, L, S), 0xA5, dtype=torch.uint8, device=gpu)
    masks = torch.full((1, S, L), -7.0, dtype=torch.float32, device=gpu)
    rc = eng.lib.dzn_prepare_masks(eng._h, C.c_void_p(raw.data_ptr()), 1, L, 21, 1, 2, C.c_void_p(filt.data_ptr()),
                                   C.c_void_p(masks.data_ptr()), eng._stream())
    torch.cuda.synchronize()
    with pytest.raises(DznError, match="invalid argument"):
        _lib.check(rc, eng._h, "dzn_prepare_masks")
    assert bool((filt == 0xA5).all()) and bool((masks == -7.0).all())


# ---- speaker_count / cluster_activations ----------------------------------------------------------------------------------
def test_count_and_cluster_aggregation_equal_integer_numpy(built_lib, gpu):
    from diarizen_amd.postprocess import _call
    for c in hc.ag_cases():
        inp = hc.ag_inputs(c)
        ref = hc.ag_run(c, inp)
        Cn, L, S, K, T = c["C"], c["L"], c["S"], c["K"], inp["T"]
        seg, hard = _dev(inp["seg"], gpu), _dev(inp["hard"], gpu)
        start = _dev(inp["start"] if Cn else np.zeros(1, np.int32), gpu)
        work = torch.full((2 * T,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        count = torch.full((T + 64,), 0xA5, dtype=torch.uint8, device=gpu)
        act = torch.full((T * K + 64,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        for _ in range(2):              # integer atomics: a second run gives the same bytes
            _call("dzn_speaker_count", seg, Cn, L, S, start, T, work, count)
            _call("dzn_cluster_activations", seg, hard, Cn, L, S, start, T, K, act)
            torch.cuda.synchronize()
            assert np.array_equal(count[:T].cpu().numpy(), ref["count"]), f"speaker count: {c}"
            assert np.array_equal(act[:T * K].cpu().numpy().reshape(T, K), ref["act"]), f"cluster activations: {c}"
            assert bool((count[T:] == 0xA5).all()) and bool((act[T * K:] == 0x5A5A5A5A).all()), f"written past the end: {c}"


# ---- hysteresis -----------------------------------------------------------------------------------------------------------
def test_hysteresis_at_the_block_edge_and_at_threshold_equality(built_lib, gpu):
    from diarizen_amd.postprocess import detect_range_launch
    for c in hc.hy_cases():
        inp = hc.hy_inputs(c)
        ref = hc.hy_run(c, inp)
        n, t0 = c["n"], c["t0"]
        entry = None if t0 == 0 else torch.tensor([c["entry"]], dtype=torch.uint8, device=gpu)
        sc, act = detect_range_launch(_dev(inp["seg"], gpu), 2, _dev(np.zeros(2, np.int32), gpu), _dev(np.ones(n, F64), gpu), t0, n, 1,
                                      c["onset"], c["offset"], entry)
        torch.cuda.synchronize()
        assert np.array_equal(sc.cpu().numpy()[:, 0], ref["scores"]), f"scores are not exactly 0 / 0.5 / 1: {c}"
        assert np.array_equal(act.cpu().numpy()[:, 0], ref["active"]), f"hysteresis differs from postprocess._hysteresis: {c}"
