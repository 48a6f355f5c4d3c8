"""The speaker registry on the device (csrc/registry.hip: registry_scan_kernel + registry_reduce_kernel through
dzn_registry_append / dzn_registry_match / ops.Registry; diarizen_amd/registry.py backend "hip"; DiariZenPipeline.link_into)
against the float64 reference

    D[k, i] = max over the rows r of identity i of cdist(q.astype(float64), E.astype(float64), "cosine")[k, r]

within the distance bound 2 (dim + 8) 2^-53 (_linking_cases.distance_bound).  Every case first asserts, on the reference alone,
that the entries of D are at least 50 bounds apart from each other and from every threshold — only then do the device's
entries <= threshold have to be exactly the reference's, and the assignments equal."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from _linking_cases import cannot_link_holds, distance_bound
from _registry_cases import GPU_CASES, GROUP_EDGES, case, columns, input_condition, seeded_registry, table

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")


def _checked_clean(lib):
    collect = getattr(lib, "dzn_checked_collect_registry", None)         # a checked build (csrc/checked.h) carries index assertions
    if collect is not None:
        words = (C.c_uint * 4)()
        assert collect(words, 0) == 0 and words[0] == 0, [hex(w) for w in words]


@pytest.mark.parametrize("n,dim,K", GPU_CASES)
def test_match_equals_the_reference_table_and_its_entries_below_the_threshold(built_lib, gpu, n, dim, K):
    from diarizen_amd import ops
    stored, ident, queries, D, ts = case(n, dim, K)            # (asserts the input condition before the device runs)
    bound = distance_bound(dim)
    reg = ops.Registry(dim, n + 3)
    try:
        reg.append(stored, ident)
        assert reg.rows == n and reg.identities == D.shape[1]
        worst = 0.0
        for t in ts:
            k, i, d, table = reg.match(queries, t, dense=True)
            assert table.shape == D.shape and table.dtype == np.float64
            finite = np.isfinite(D)
            assert np.array_equal(np.isinf(table) & (table > 0), ~finite)      # +inf exactly at the numbers without a row
            worst = max(worst, float(np.abs(table[finite] - D[finite]).max()))
            want = {(int(a), int(b)) for a, b in zip(*np.nonzero(D <= t))}
            assert set(zip(k.tolist(), i.tolist())) == want and len(k) == len(want), t
            assert np.array_equal(d, table[k, i])                              # the triples carry the table's own bits
            assert list(zip(k.tolist(), i.tolist())) == sorted(want)
            k2, i2, d2 = reg.match(queries, t)                                 # without the dense table: the same triples
            assert np.array_equal(k, k2) and np.array_equal(i, i2) and np.array_equal(d.view(np.uint64), d2.view(np.uint64))
            k3, i3, d3 = reg.match(queries, t, max_out=1)                      # too little room: asked again with enough
            assert np.array_equal(k, k3) and np.array_equal(i, i3) and np.array_equal(d, d3)
        print(f"registry match n {n} dim {dim} K {K}: worst |d - scipy| {worst:.3e} (bound {bound:.3e})")
        assert worst <= bound
        assert reg.last_launch_ms() > 0.0
    finally:
        reg.close()
    _checked_clean(built_lib)


@pytest.mark.parametrize("n,dim,K", [(65, 20, 33), (257, 256, 31), (513, 16, 2), (513, 256, 33)] +
                         [(n, dim, k) for n, dim in ((65, 20), (513, 256)) for k in GROUP_EDGES])
def test_appending_in_pieces_and_matching_twice_give_the_same_bits(built_lib, gpu, n, dim, K):
    from diarizen_amd import ops
    stored, ident, queries, D, ts = case(n, dim, K)
    whole, pieces = ops.Registry(dim, n), ops.Registry(dim, n)
    try:
        whole.append(stored, ident)
        cuts = [0, 1, min(n, 64), min(n, 65), min(n, 200), n]
        seen = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            pieces.append(stored[a:b], ident[a:b])                            # (an empty piece is a no-op)
            if b > a:
                seen.append(pieces.match(queries, 2.0, dense=True)[3])        # a match between appends: the index is rebuilt
        assert pieces.rows == n
        for t in ts[1:]:
            a = whole.match(queries, t, dense=True)
            b = pieces.match(queries, t, dense=True)
            c = whole.match(queries, t, dense=True)
            for x, y, z in zip(a, b, c):
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                assert np.array_equal(x.view(np.uint8), z.view(np.uint8))
        # the result of a query does not depend on the group it travels in: one at a time, all at once
        solo = np.concatenate([whole.match(queries[q:q + 1], 2.0, dense=True)[3] for q in range(K)])
        assert np.array_equal(solo.view(np.uint64), whole.match(queries, 2.0, dense=True)[3].view(np.uint64))
        assert np.array_equal(seen[-1].view(np.uint64), solo.view(np.uint64))
    finally:
        whole.close()
        pieces.close()
    _checked_clean(built_lib)


@pytest.mark.parametrize("n,dim", [(65, 20), (513, 256)])
def test_registry_hip_equals_numpy_over_a_sequence_of_adds(built_lib, gpu, n, dim):
    """adds of 1, 33, 2, 40 and 31 labels onto a seeded registry: the stored rows cross the 64-entry chunk, the new rows the
    32-query group; identities equal exactly, diameters within the bound"""
    from _linking_cases import planted
    stored, ident, queries, D, ts = case(n, dim, 33)
    t = ts[1]
    extra = planted(1 + 33 + 2 + 40 + 31, dim, 7)
    ref, _ = seeded_registry(stored, ident, t, "numpy", dim, capacity=n + 256)
    dev, _ = seeded_registry(stored, ident, t, "hip", dim, capacity=n + 256)
    try:
        at = 0
        for j, K in enumerate((1, 33, 2, 40, 31)):
            rows = queries if K == 33 else extra[at:at + K]
            at += 0 if K == 33 else K
            T = table(rows, ref.rows, ref.row_identity, ref.num_identities)      # the input condition of this add
            assert input_condition(T[:, columns(T)], [t], dim) >= 50.0
            a, b = ref.add(f"new{j}", rows), dev.add(f"new{j}", rows)
            assert a == b and ref.identity == dev.identity
            assert set(ref.diameter) == set(dev.diameter)
            assert max(abs(ref.diameter[i] - dev.diameter[i]) for i in ref.diameter) <= distance_bound(dim)
            assert cannot_link_holds(dev.links())
        assert ref.device_calls == 0 and dev.device_calls == 5 and dev.links().backend == "hip"
        assert np.array_equal(ref.rows, dev.rows) and np.array_equal(ref.row_identity, dev.row_identity)
        assert len(set(ref.identity.values())) < len(ref.identity)            # something joined
    finally:
        dev.close()
    _checked_clean(built_lib)


def test_auto_takes_the_device_from_the_row_count_up(built_lib, gpu, monkeypatch):
    from diarizen_amd import registry
    stored, ident, queries, D, ts = case(65, 20, 2)
    monkeypatch.setattr(registry, "REGISTRY_HIP_MIN", 65)
    reg, _ = seeded_registry(stored[:64], ident[:64], ts[1], "auto", 20)
    try:
        reg.add("a", stored[64:65])
        assert reg.device_calls == 0 and len(reg) == 65
        reg.add("b", queries)
        assert reg.device_calls == 1 and reg.links().backend == "hip"
    finally:
        reg.close()
    odd = registry.SpeakerRegistry(0.5, dim=18, backend="auto")              # a dim the device refuses: "auto" stays on the host
    monkeypatch.setattr(registry, "REGISTRY_HIP_MIN", 1)
    odd.add("a", np.ones((1, 18), np.float32))
    with pytest.warns(UserWarning, match="device path failed"):
        assert odd.add("b", np.ones((1, 18), np.float32)) == {0: 0}
    assert odd.links().backend == "numpy" and odd.device_error.startswith("DznError")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                        # given up for good: not tried, not warned again
        assert odd.add("c", np.ones((1, 18), np.float32)) == {0: 0}
    hip = registry.SpeakerRegistry(0.5, dim=18, backend="hip")
    hip.add("a", np.ones((1, 18), np.float32))
    from diarizen_amd._lib import DznError
    with pytest.raises(DznError):
        hip.add("b", np.ones((1, 18), np.float32))
    assert len(hip) == 1 and hip.num_identities == 1                          # the refused add changed nothing


def test_refusals_through_the_c_abi_write_nothing(built_lib, gpu):
    lib = built_lib
    dim, cap = 16, 6
    r = np.random.default_rng(0)
    rows = r.standard_normal((4, dim)).astype(np.float32)
    ident = np.array([0, 2, 0, 5], dtype=np.int32)
    q = r.standard_normal((3, dim)).astype(np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.dzn_registry_create(-1, dim, cap, None) == -1
    for d_, c_ in ((0, cap), (18, cap), (2048, cap), (dim, 0)):
        assert lib.dzn_registry_create(-1, d_, c_, C.byref(h)) == -1 and not h
    assert lib.dzn_registry_create(-1, dim, cap, C.byref(h)) == 0 and h
    try:
        n, I = C.c_int64(-7), C.c_int64(-7)
        k, i, d = np.full(8, -7, np.int32), np.full(8, -7, np.int32), np.full(8, -7.0)
        m = C.c_int32(-7)
        dense = np.full((3, 6), -7.0)

        def match(hh=h, qq=p(q), Q=3, t=2.0, room=8, kk=p(k), ii=p(i), dd=p(d), mm=C.byref(m), de=p(dense)):
            return lib.dzn_registry_match(hh, qq, Q, t, room, kk, ii, dd, mm, de)

        assert match() == 0 and m.value == 0 and (dense == -7.0).all()        # an empty registry: no launch, nothing but the count
        m.value = -7
        assert lib.dzn_registry_append(h, p(rows), 4, p(ident)) == 0
        assert lib.dzn_registry_rows(h, C.byref(n), C.byref(I)) == 0 and (n.value, I.value) == (4, 6)
        assert lib.dzn_registry_rows(h, C.byref(n), None) == 0 and lib.dzn_registry_rows(h, None, None) == -1
        # append refusals: null pointers, a negative count, a bad identity number, a row without a direction, no room left
        bad_id, zero, nan = ident[:2].copy(), rows[:2].copy(), rows[:2].copy()
        bad_id[1], zero[1], nan[0, 3] = -1, 0.0, np.nan
        assert lib.dzn_registry_append(None, p(rows), 2, p(ident)) == -1
        assert lib.dzn_registry_append(h, None, 2, p(ident)) == -1 and lib.dzn_registry_append(h, p(rows), 2, None) == -1
        assert lib.dzn_registry_append(h, p(rows), -1, p(ident)) == -1
        assert lib.dzn_registry_append(h, p(rows), 2, p(bad_id)) == -1
        assert lib.dzn_registry_append(h, p(zero), 2, p(ident)) == -1 and lib.dzn_registry_append(h, p(nan), 2, p(ident)) == -1
        assert lib.dzn_registry_append(h, p(rows), 3, p(ident)) == -2          # capacity exceeded
        assert lib.dzn_registry_append(h, p(rows), 0, p(ident)) == 0
        assert lib.dzn_registry_rows(h, C.byref(n), C.byref(I)) == 0 and (n.value, I.value) == (4, 6)
        # match refusals
        qz, qn = q.copy(), q.copy()
        qz[2], qn[0, 0] = 0.0, np.inf
        assert match(hh=None) == -1 and match(qq=None) == -1 and match(mm=None) == -1
        assert match(kk=None) == -1 and match(ii=None) == -1 and match(dd=None) == -1
        assert match(Q=-1) == -1 and match(room=-1) == -1
        assert match(qq=p(qz)) == -1 and match(qq=p(qn)) == -1
        for t in (0.0, -0.5, 2.0000001, float("nan"), float("inf")):
            assert match(t=t) == -1
        assert m.value == -7 and (k == -7).all() and (i == -7).all() and (d == -7.0).all() and (dense == -7.0).all()
        ms = C.c_float(-7.0)
        assert lib.dzn_registry_last_launch_ms(h, C.byref(ms)) == -4 and ms.value == -7.0      # nothing was launched yet
        # and the registry still answers: everything is <= 2.0, the refused rows are not in it
        assert match() == 0 and m.value == 9 and sorted(set(i[:8].tolist())) == [0, 2, 5]
        assert np.isinf(dense[:, [1, 3, 4]]).all() and np.isfinite(dense[:, [0, 2, 5]]).all()
        assert match(Q=0, qq=None) == 0 and m.value == 0
        assert match(room=0, kk=None, ii=None, dd=None) == 0 and m.value == 9  # the count alone
        assert lib.dzn_registry_last_launch_ms(h, C.byref(ms)) == 0 and ms.value > 0.0
    finally:
        assert lib.dzn_registry_destroy(h) == 0
    assert lib.dzn_registry_destroy(None) == 0
    _checked_clean(built_lib)


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


def test_link_into_pairs_a_recording_with_itself(built_lib, gpu, pipe, tmp_path):
    """the same recording under two names at threshold 2.0 (everything allowed merges): label k of "b" joins the identity of
    label k of "a" — the smallest entries are the zeros of equal centroids — and two labels of one recording still differ"""
    from diarizen_amd.registry import SpeakerRegistry
    reg = SpeakerRegistry(2.0, dim=256, capacity=64, device=gpu, backend="hip")
    pipe.rttm_out_dir = str(tmp_path)
    try:
        got = list(pipe.link_into(reg, [WAV, WAV], sess_names=["a", "b"]))
    finally:
        pipe.rttm_out_dir = None
    try:
        assert [g[0] for g in got] == ["a", "b"]
        K = len(got[0][2])
        assert K >= 2 and got[0][2] == got[1][2] == {k: k for k in range(K)}
        assert reg.num_identities == K and len(reg) == 2 * K and reg.unusable == [] and reg.device_calls == 1
        assert cannot_link_holds(reg.links()) and all(reg.diameter[k] <= 1e-6 for k in range(K))
        for name, ann, ids in got:
            labels = {lab for _, _, lab in ann.itertracks(yield_label=True)}
            assert labels == {f"spk{k:04d}" for k in range(K)}
            assert (tmp_path / f"{name}.rttm").read_text() == ann.to_rttm()
    finally:
        reg.close()
    _checked_clean(built_lib)
