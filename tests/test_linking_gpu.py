"""Linking speakers across recordings on the device (csrc/linkage.hip: pdist_cosine_group_kernel + step2_kernel<RULE_COMPLETE>
through dzn_link_speakers / ops.link_speakers; diarizen_amd/linking.py; DiariZenPipeline.link_many) against the scipy
definition

    y = pdist(E.astype(float64), "cosine");  y[same group] = 4.0;  Z = linkage(y, "complete")

The first m rows of the device's Z are the merges of height <= t: ids and sizes equal exactly, heights within the distance
bound 2 (dim + 8) 2^-53 (_linking_cases.distance_bound).  Every case first asserts, on the reference alone, that its allowed
distances are at least 50 bounds apart from each other and from every threshold — only then can neither side's rounding
reorder two merges."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from _linking_cases import DIMS, LAYOUTS, ROWS, cannot_link_holds, case, distance_bound, linker_for

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")


def _checked_clean(lib):
    collect = getattr(lib, "dzn_checked_collect_linkage", None)          # a checked build (csrc/checked.h) carries index assertions
    if collect is not None:
        words = (C.c_uint * 4)()
        assert collect(words, 0) == 0 and words[0] == 0, [hex(w) for w in words]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", ROWS)
def test_link_speakers_equals_the_scipy_definition(built_lib, gpu, n, dim, layout):
    from diarizen_amd import ops
    emb, group, Z, ts = case(n, dim, layout)          # (asserts the input condition before the device runs)
    bound = distance_bound(dim)
    worst = 0.0
    for t in ts:
        want = int(np.count_nonzero(Z[:, 2] <= t))
        got, m = ops.link_speakers(emb, group, t)
        assert m == want and got.shape == (m, 4) and got.dtype == np.float64, (t, m, want)
        assert np.array_equal(got[:, [0, 1, 3]], Z[:m][:, [0, 1, 3]]), t
        if m:
            worst = max(worst, float(np.abs(got[:, 2] - Z[:m, 2]).max()))
        stats = ops.link_speakers_last()
        assert stats["merges"] == m and stats["launches"] >= m + stats["rescans"]
    print(f"link_speakers n {n} dim {dim} {layout}: worst |height - scipy| {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    if layout == "one_group":
        assert all(int(np.count_nonzero(Z[:, 2] <= t)) == 0 for t in ts)
    _checked_clean(built_lib)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,dim", [(3, 16), (65, 20), (257, 256), (513, 16)])
def test_linker_hip_equals_scipy_in_identity(built_lib, gpu, n, dim, layout):
    emb, group, Z, ts = case(n, dim, layout)
    for t in ts:
        ref, _ = linker_for(emb, group, t, "scipy", dim)
        dev, _ = linker_for(emb, group, t, "hip", dim)
        a, b = ref.link(), dev.link()
        usable = len(emb) >= 2
        assert a.backend == ("scipy" if usable else "trivial") and b.backend == ("hip" if usable else "trivial")
        assert ref.device_calls == 0 and dev.device_calls == int(usable)
        assert a.identity == b.identity and a.num_identities == b.num_identities
        assert cannot_link_holds(a) and cannot_link_holds(b)
        assert set(a.diameter) == set(b.diameter)
        assert max(abs(a.diameter[i] - b.diameter[i]) for i in a.diameter) <= distance_bound(dim)
    _checked_clean(built_lib)


def test_refusals_and_the_memory_error(built_lib, gpu, monkeypatch):
    from diarizen_amd import ops
    from diarizen_amd._lib import DznError
    lib = built_lib
    n, dim = 5, 16
    emb = np.random.default_rng(0).standard_normal((n, dim)).astype(np.float32)
    group = np.arange(n, dtype=np.int32)
    Z = np.full((n - 1, 4), -7.0)
    m = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(e=emb, g=group, n_=n, dim_=dim, t=0.5, z=Z, mm=C.byref(m)):
        return lib.dzn_link_speakers(p(e) if e is not None else None, p(g) if g is not None else None, n_, dim_, t,
                                     p(z) if z is not None else None, mm, -1)

    assert call(e=None) == -1 and call(g=None) == -1 and call(z=None) == -1 and call(mm=None) == -1
    assert call(n_=1) == -1 and call(n_=0) == -1 and call(dim_=0) == -1
    for t in (0.0, -0.5, 2.0000001, float("nan"), float("inf")):
        assert call(t=t) == -1
    zero, nan, inf = emb.copy(), emb.copy(), emb.copy()
    zero[3], nan[3, 2], inf[4, 15] = 0.0, np.nan, np.inf
    assert call(e=zero) == -1 and call(e=nan) == -1 and call(e=inf) == -1
    assert (Z == -7.0).all() and m.value == -7                          # nothing written by a refused call
    assert call(t=2.0) == 0 and 0 <= m.value <= n - 1
    with pytest.raises(DznError):
        ops.link_speakers(emb, group, 0.0)
    with pytest.raises(ValueError):
        ops.link_speakers(emb, group[:-1], 0.5)
    monkeypatch.setattr(lib, "dzn_link_speakers", lambda *a: -2)        # DZN_E_NOMEM: the n x n matrix did not fit
    with pytest.raises(MemoryError):
        ops.link_speakers(emb, group, 0.5)
    # "auto" falls back to scipy on it, "hip" raises
    from diarizen_amd import linking
    monkeypatch.setattr(linking, "HIP_LINK_MIN", 2)
    L, _ = linker_for(emb, group, 0.5, "auto", dim)
    assert L.link().backend == "scipy" and L.device_calls == 1
    L, _ = linker_for(emb, group, 0.5, "hip", dim)
    with pytest.raises(MemoryError):
        L.link()


def test_auto_takes_scipy_for_bit_identical_rows(built_lib, gpu, monkeypatch):
    from diarizen_amd import linking
    monkeypatch.setattr(linking, "HIP_LINK_MIN", 8)
    emb, group, Z, ts = case(65, 20, "groups_3_4")
    L, _ = linker_for(emb, group, ts[1], "auto", 20)
    assert L.link().backend == "hip" and L.device_calls == 1
    dup = np.array(emb, copy=True)
    dup[40] = dup[2]                                                    # an exact tie (rows of two different groups)
    L, _ = linker_for(dup, group, ts[1], "auto", 20)
    links = L.link()
    assert links.backend == "scipy" and L.device_calls == 0
    assert cannot_link_holds(links)
    few, _ = linker_for(emb[:6], group[:6], ts[1], "auto", 20)         # below the row count: scipy
    assert few.link().backend == "scipy" and few.device_calls == 0


# ----------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    p = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield p
    p.close()


@pytest.fixture(scope="module")
def single(pipe):
    """`__call__(return_embeddings=True)` on the recording, once"""
    return pipe(WAV, sess_name="EN2002a", return_embeddings=True)


def test_diarize_many_return_embeddings(built_lib, gpu, pipe, single):
    ann, cent = single
    plain = list(pipe.diarize_many([WAV, WAV], sess_names=["a", "b"]))
    assert [len(t) for t in plain] == [2, 2] and [t[0] for t in plain] == ["a", "b"]         # the parent's tuples
    assert all(t[1].to_rttm() == ann.to_rttm().replace(" EN2002a ", f" {t[0]} ") for t in plain)
    for overlap in (True, False):
        got = list(pipe.diarize_many([WAV, WAV], sess_names=["a", "b"], overlap=overlap, return_embeddings=True))
        assert [len(t) for t in got] == [3, 3]
        for (name, a, c), (_, a0) in zip(got, plain):
            assert a.to_rttm() == a0.to_rttm()
            assert c.dtype == np.float32 and c.shape == cent.shape and np.array_equal(c.view(np.uint32), cent.view(np.uint32))
    both = list(pipe.diarize_many([WAV], sess_names=["a"], return_scores=True, return_embeddings=True))
    assert len(both[0]) == 4 and np.array_equal(both[0][3], cent) and both[0][2].data.shape[1] == len(cent)


@pytest.mark.parametrize("threshold", [1e-6, 1.9])
def test_link_many_pairs_a_recording_with_itself(built_lib, gpu, pipe, single, tmp_path, threshold):
    """the same recording twice: label k of "a" and label k of "b" are one identity — at 1e-6 because their centroids are
    equal, at 1.9 because nothing else may join them: the other candidates are labels of the same two recordings"""
    ann, cent = single
    K = len(cent)
    assert K >= 2
    pipe.rttm_out_dir = str(tmp_path)
    try:
        out, links = pipe.link_many([WAV, WAV], threshold=threshold, sess_names=["a", "b"])
    finally:
        pipe.rttm_out_dir = None
    assert links.num_identities == K and cannot_link_holds(links) and links.unusable == []
    assert all(links.identity[("a", k)] == links.identity[("b", k)] == k for k in range(K))
    assert all(links.diameter[k] <= 1e-6 for k in range(K))
    for name in ("a", "b"):
        want = ann.to_rttm().replace(" EN2002a ", f" {name} ")
        for k in range(K):
            want = want.replace(f"<NA> <NA> {k} <NA> <NA>\n", f"<NA> <NA> spk{k:04d} <NA> <NA>\n")
        assert out[name].to_rttm() == want and (tmp_path / f"{name}.rttm").read_text() == want
    with pytest.raises(ValueError):
        pipe.link_many([WAV, WAV], threshold=threshold, sess_names=["a", "a"])
