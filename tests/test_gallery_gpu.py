"""The device gallery (csrc/gallery.hip: dzn_gallery_*, ops.GalleryState, identification.SpeakerGallery) on the MI355X against
the float64 restatement of tests/_gallery_cases.py: every score within the derived bound B(dim) at the tile, sweep and query-group
edges, the selection equal to the order (score descending, slot ascending) of the same call's dense output bit for bit, planted
matches, drops and re-puts, growth, the search counter and the ABI's refusals.  tile_rows / sweep_rows / query_group come from
dzn_gallery_geometry."""
import ctypes as C

import numpy as np
import pytest

from _gallery_cases import bound, gallery_case, planted_case, ref_scores, select

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(built_lib, gpu):
    from diarizen_amd import ops
    g = ops.GalleryState(16, 1)
    out = dict(t=g.tile_rows, s=g.sweep_rows, g=g.query_group, n=g.max_top_n)
    g.close()
    assert out["t"] >= 16 and out["s"] % out["t"] == 0 and out["g"] % 16 == 0 and out["n"] == 32
    return out


def size(expr: str, geo) -> int:
    """"2t+3", "s-1", "g+1", "17" -> the number, with t / s / g from the geometry"""
    return int(eval(expr.replace("2t", "2*t").replace("2g", "2*g"), {}, dict(geo)))


def check_selection(scores, slots, dense, top_n):
    exp_s, exp_i = select(dense, top_n)
    assert np.array_equal(slots, exp_i)
    assert np.array_equal(scores.view(np.uint32), exp_s.view(np.uint32))        # bit for bit (-inf tails included)


# (rows, Q, dim): every row count and every Q of the issue's lists once or more, the large row counts with small Q
DENSE = [("1", "2g+1", 256), ("15", "g+1", 16), ("16", "g", 512), ("17", "g-1", 256),
         ("t-1", "17", 512), ("t", "16", 256), ("t+1", "15", 16), ("2t+3", "g+1", 512), ("2t+3", "1", 16),
         ("s-1", "1", 256), ("s", "16", 256), ("s+1", "17", 256), ("s+1", "1", 512), ("s+1", "2", 16)]


@pytest.mark.parametrize("rows,Q,dim", DENSE)
def test_dense_scores_within_the_bound_and_selection_follows_them(geo, rows, Q, dim):
    from diarizen_amd import ops
    n, nq = size(rows, geo), size(Q, geo)
    r, q = gallery_case(1000 + n + 7 * nq + dim, n, nq, dim)
    ref = ref_scores(r, q)
    g = ops.GalleryState(dim, n)
    try:
        g.put(0, r)
        assert g.rows == n
        top_n = 16
        scores, slots, dense = g.search(q, top_n, dense=True)
    finally:
        g.close()
    assert dense.shape == (nq, n) and dense.dtype == np.float32 and np.isfinite(dense).all()
    err = float(np.max(np.abs(dense.astype(np.float64) - ref)))
    print(f"rows {n} Q {nq} dim {dim}: max |score - float64| = {err:.3e}, bound {bound(dim):.3e}")
    assert err <= bound(dim)
    check_selection(scores, slots, dense, top_n)


@pytest.mark.parametrize("top_n", [1, 2, 16, 32])
def test_selection_order_ties_and_the_last_slot(geo, top_n):
    """duplicated rows in one tile, in two tiles of one workgroup (a sweep apart) and in tiles of different workgroups tie and
    the lower slot comes first; the best row of a query sits in the last slot"""
    from diarizen_amd import ops
    t, s = geo["t"], geo["s"]
    dim, n = 16, s + t + 3
    r, _ = gallery_case(77, n, 1, dim, scaled=False)
    r[9] = r[3]                      # one tile
    r[5 + s] = r[5]                  # tile 0 and tile s / t: the same workgroup, one sweep later
    r[t + 7] = r[7]                  # tiles 0 and 1: different workgroups
    q = np.stack([r[3], r[5], r[7], r[n - 1], r[11] + r[12]])
    g = ops.GalleryState(dim, n)
    try:
        g.put(0, r)
        scores, slots, dense = g.search(q, top_n, dense=True)
    finally:
        g.close()
    check_selection(scores, slots, dense, top_n)
    assert slots[3, 0] == n - 1
    if top_n >= 2:
        assert list(slots[0, :2]) == [3, 9] and list(slots[1, :2]) == [5, 5 + s] and list(slots[2, :2]) == [7, t + 7]
        for k in range(3):
            assert scores[k, 0] == scores[k, 1]
    else:
        assert list(slots[:3, 0]) == [3, 5, 7]


@pytest.mark.parametrize("top_n", [5, 16, 32])
def test_top_n_at_and_beyond_the_number_of_valid_rows(geo, top_n):
    from diarizen_amd import ops
    dim, n = 256, 7
    r, q = gallery_case(5, n, 3, dim)
    g = ops.GalleryState(dim, 40)
    try:
        g.put(0, r)
        g.drop(1, 2)                 # 5 valid rows
        scores, slots, dense = g.search(q, top_n, dense=True)
    finally:
        g.close()
    check_selection(scores, slots, dense, top_n)
    assert (slots[:, :5] >= 0).all() and (slots[:, 5:] == -1).all() and np.isneginf(scores[:, 5:]).all()
    assert np.isneginf(dense[:, 1:3]).all() and not np.isin(slots, [1, 2]).any()


def test_planted_matches(geo):
    from diarizen_amd import ops
    dim, n, Q = 256, 3 * geo["t"] + 11, geo["g"] + 3
    r, q, at = planted_case(11, n, Q, dim)
    ref = ref_scores(r, q)
    top2 = np.sort(ref, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    assert (np.argmax(ref, axis=1) == at).all() and margin.min() >= 0.1       # far above 2 B: no case is left out
    g = ops.GalleryState(dim, n)
    try:
        g.put(0, r)
        scores, slots = g.search(q, 1)
    finally:
        g.close()
    assert np.array_equal(slots[:, 0], at)
    assert np.max(np.abs(scores[:, 0] - ref[np.arange(Q), at])) <= bound(dim)


def test_drops_and_reputs(geo):
    from diarizen_amd import ops
    t = geo["t"]
    dim, n = 256, 3 * t
    r, q = gallery_case(21, n, 4, dim)
    valid = np.ones(n, dtype=bool)
    g = ops.GalleryState(dim, n + 5)
    try:
        g.put(0, r)

        def check():
            scores, slots, dense = g.search(q, 16, dense=True)
            ref = ref_scores(r, q, valid)
            assert np.array_equal(np.isneginf(dense), np.isneginf(ref))      # -inf exactly at the dropped slots
            ok = ~np.isneginf(ref)
            assert np.max(np.abs(dense[ok] - ref[ok]), initial=0.0) <= bound(dim)
            check_selection(scores, slots, dense, 16)
            assert not np.isin(slots, np.nonzero(~valid)[0]).any()
            return slots

        best = int(check()[0, 0])
        g.drop(best)                                     # the best match of query 0
        valid[best] = False
        assert check()[0, 0] != best
        g.drop(t, t)                                     # a whole tile
        valid[t:2 * t] = False
        check()
        g.put(best, r[best])                             # a dropped slot comes back
        valid[best] = True
        assert check()[0, 0] == best
        other = 7 if best != 7 else 8
        r[other] = r[best]                               # put over a live slot replaces it
        g.put(other, r[other])
        slots = check()
        assert list(slots[0, :2]) == sorted([other, best])
        g.drop(0, n)                                     # every row but one
        valid[:] = False
        g.put(2 * t + 1, r[2 * t + 1])
        valid[2 * t + 1] = True
        slots = check()
        assert (slots[:, 0] == 2 * t + 1).all() and (slots[:, 1:] == -1).all()
        g.drop(2 * t + 1)                                # every row
        valid[:] = False
        slots = check()
        assert (slots == -1).all()
    finally:
        g.close()


def test_growth_gives_the_answers_of_a_gallery_created_large(geo, gpu):
    from diarizen_amd.identification import SpeakerGallery
    dim, n = 256, 70
    r, q = gallery_case(31, n, 5, dim)
    small, large = SpeakerGallery(dim, gpu, capacity=4), SpeakerGallery(dim, gpu, capacity=256)
    try:
        for i in range(10):
            small.enroll(f"p{i}", r[i])
        s0, n0 = small.search(q, 3)                      # the device state exists at capacity 16 ...
        for i in range(10, n):
            small.enroll(f"p{i}", r[i])                  # ... and is replaced by a larger one
        for i in range(n):
            large.enroll(f"p{i}", r[i])
        assert small.capacity == 128 and large.capacity == 256
        a, b = small.search(q, 8), large.search(q, 8)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        ref_s, ref_i = select(ref_scores(r, q), 8)
        assert a[1] == [[f"p{i}" for i in row] for row in ref_i]
        assert s0.shape == (5, 3) and all(nm in {f"p{i}" for i in range(10)} for row in n0 for nm in row)
    finally:
        small.close()
        large.close()


def test_searches_counter_and_unusable_queries(geo, gpu):
    from diarizen_amd.identification import SpeakerGallery
    dim = 256
    r, q = gallery_case(41, 6, 4, dim)
    g = SpeakerGallery(dim, gpu)
    try:
        for i in range(6):
            g.enroll(f"n{i}", r[i])
        assert g.searches == 0
        g.search(q, 2)
        assert g.searches == 1
        bad = q.copy()
        bad[1] = 0.0
        bad[2, 5] = np.nan
        scores, names = g.search(bad, 2)
        assert g.searches == 2
        assert names[1] == [None, None] and names[2] == [None, None] and np.isneginf(scores[1:3]).all()
        good_s, good_n = g.search(q[[0, 3]], 2)
        assert names[0] == good_n[0] and names[3] == good_n[1] and np.array_equal(scores[[0, 3]], good_s)
        g.search(bad[1:3], 2)                            # nothing usable: no library call
        assert g.searches == 3
        g.remove("n0")
        _, names = g.search(r[:1], 6)
        assert "n0" not in names[0] and names[0][5] is None and g.searches == 4
    finally:
        g.close()


def test_abi_refusals_leave_the_outputs_alone(built_lib, geo):
    lib = built_lib
    dim, cap = 32, 10
    vp = C.c_void_p
    h = vp()
    for bad_dim, bad_cap in ((8, cap), (24, cap), (528, cap), (dim, 0)):
        assert lib.dzn_gallery_create(-1, bad_dim, bad_cap, C.byref(h)) == -1 and not h
    assert lib.dzn_gallery_create(-1, dim, cap, None) == -1
    assert lib.dzn_gallery_create(-1, dim, cap, C.byref(h)) == 0
    try:
        r, q = gallery_case(51, 4, 2, dim, scaled=False)
        ptr = lambda a: a.ctypes.data_as(vp)
        assert lib.dzn_gallery_put(h, 0, ptr(r), 4) == 0
        scores = np.full((2, 3), 7.5, dtype=np.float32)
        slots = np.full((2, 3), -77, dtype=np.int64)
        dense = np.full((2, 4), 7.5, dtype=np.float32)

        def untouched():
            return (scores == 7.5).all() and (slots == -77).all() and (dense == 7.5).all()

        def search(handle=h, qp=None, Q=2, n=3, sp=None, ip=None):
            return lib.dzn_gallery_search(handle, ptr(q) if qp is None else qp, Q, n, ptr(scores) if sp is None else sp,
                                          ptr(slots) if ip is None else ip, ptr(dense))

        assert search(handle=None) == -1 and search(qp=vp()) == -1 and search(sp=vp()) == -1 and search(ip=vp()) == -1
        assert search(Q=0) == -1 and search(n=0) == -1 and search(n=geo["n"] + 1) == -1
        for value in (np.nan, np.inf):
            bad = q.copy()
            bad[1, 3] = value
            assert search(qp=ptr(bad)) == -1
        bad = q.copy()
        bad[0] = 0.0
        assert search(qp=ptr(bad)) == -1
        assert untouched()
        # put: null, ranges outside the capacity, zero / non-finite rows (none of the rows of a refused put is stored)
        assert lib.dzn_gallery_put(None, 0, ptr(r), 1) == -1 and lib.dzn_gallery_put(h, 0, None, 1) == -1
        assert lib.dzn_gallery_put(h, -1, ptr(r), 1) == -1 and lib.dzn_gallery_put(h, cap - 3, ptr(r), 4) == -1
        assert lib.dzn_gallery_put(h, 0, ptr(r), 0) == -1 and lib.dzn_gallery_put(h, cap, ptr(r), 1) == -1
        for value in (np.nan, -np.inf, 0.0):
            bad = r[::-1].copy()
            bad[3] = value if value == 0.0 else bad[3]
            bad[3, 0] = value
            assert lib.dzn_gallery_put(h, 0, ptr(bad), 4) == -1
        assert lib.dzn_gallery_drop(h, -1, 1) == -1 and lib.dzn_gallery_drop(h, cap - 1, 2) == -1
        assert lib.dzn_gallery_drop(None, 0, 1) == -1 and lib.dzn_gallery_drop(h, 0, 0) == -1
        g4 = [C.c_int32(0) for _ in range(4)]
        assert lib.dzn_gallery_geometry(None, *[C.byref(v) for v in g4]) == -1
        assert lib.dzn_gallery_geometry(h, None, C.byref(g4[1]), C.byref(g4[2]), C.byref(g4[3])) == -1
        assert untouched()
        assert search() == 0                             # the gallery still holds the first put, and only that
        exp_s, exp_i = select(dense, 3)
        assert np.array_equal(slots, exp_i) and np.array_equal(scores, exp_s)
        assert np.max(np.abs(dense - ref_scores(r, q))) <= bound(dim)
    finally:
        assert lib.dzn_gallery_destroy(h) == 0
    assert lib.dzn_gallery_destroy(None) == 0
