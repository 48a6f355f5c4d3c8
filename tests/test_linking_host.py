"""Linking speakers across recordings, the parts that need no GPU (diarizen_amd/linking.py): a numpy model of the device
loop's step rules under the complete-linkage update and the stop test against the scipy definition, and the known answers of
SpeakerLinker(backend="scipy")."""
import os

import numpy as np
import pytest

from _linking_cases import BIG, cannot_link_holds, case, definition, groups, planted


# ----------------------------------------------------------------------------- the device loop, as an algorithm
def _link_top2_model(D, threshold):
    """Row-level numpy model of csrc/linkage.hip's step2_kernel<RULE_COMPLETE> on a full masked distance matrix D (diagonal
    +inf): the two remembered neighbours per row of tests/test_design_math.py::_linkage_top2_model
       I1: l1 <= D[z][c] for every active c != z;            e1: D[z][n1] == l1
       I2: l2 <= D[z][c] for every active c not in {z, n1};  e2: D[z][n2] == l2
    with the update v = max(d_xi, d_yi) and the stop at the first winning bound above the threshold, exact or stale.
    -> (Z prefix, merges, steps, rescans)"""
    INF = np.inf
    D = np.array(D, dtype=np.float64, copy=True)
    n = len(D)
    size = np.ones(n, np.int64)
    cid = np.arange(n)
    Z = np.zeros((n - 1, 4))
    l1, l2 = np.zeros(n), np.zeros(n)
    n1, n2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    e1, e2 = np.ones(n, bool), np.ones(n, bool)

    def top2_of(row, mask):
        v = np.where(mask, row, INF)
        i1 = int(np.argmin(v))
        v1 = v[i1]
        v[i1] = INF
        i2 = int(np.argmin(v))
        v2 = v[i2]
        return v1, (i1 if np.isfinite(v1) else -1), v2, (i2 if np.isfinite(v2) else -1)

    for z in range(n):
        l1[z], n1[z], l2[z], n2[z] = top2_of(D[z], size != 0)
        e1[z], e2[z] = n1[z] >= 0, n2[z] >= 0
    k = steps = rescans = 0
    while k < n - 1:
        steps += 1
        assert steps < 4 * n + 8
        lbm = np.where(size != 0, l1, INF)
        xw = int(np.argmin(lbm))
        d = lbm[xw]
        assert np.isfinite(d)
        if d > threshold:                                  # STOP: a lower bound of everything left
            act = size != 0
            assert D[np.ix_(act, act)].min() >= d
            break
        if not (e1[xw] and n1[xw] >= 0):                   # RESCAN: refills both slots
            rescans += 1
            l1[xw], n1[xw], l2[xw], n2[xw] = top2_of(D[xw], size != 0)
            e1[xw], e2[xw] = n1[xw] >= 0, n2[xw] >= 0
            continue
        y = int(n1[xw])
        assert D[xw, y] == d
        lo, hi = (xw, y) if xw < y else (y, xw)
        nlo, nhi = int(size[lo]), int(size[hi])
        Z[k] = (min(cid[lo], cid[hi]), max(cid[lo], cid[hi]), d, nlo + nhi)
        newrow = np.full(n, INF)
        size[lo] = 0
        for z in range(n):
            if z == hi or z == lo or size[z] == 0:
                continue
            v = max(D[lo, z], D[hi, z])                    # the one line that differs from the centroid rule
            newrow[z] = v
            D[hi, z] = D[z, hi] = v
            d1 = n1[z] in (lo, hi)
            d2 = n2[z] in (lo, hi)
            if not d1:
                if v < l1[z]:
                    l2[z], n2[z], e2[z] = l1[z], n1[z], e1[z]
                    l1[z], n1[z], e1[z] = v, hi, True
                elif not d2:
                    if v < l2[z]:
                        l2[z], n2[z], e2[z] = v, hi, True
                elif v <= l2[z]:
                    l2[z], n2[z], e2[z] = v, hi, True
                else:
                    n2[z], e2[z] = hi, False
            elif not d2 and e2[z]:
                if v < l2[z]:
                    l1[z], n1[z], e1[z] = v, hi, True
                else:
                    l1[z], n1[z], e1[z] = l2[z], n2[z], True
                    n2[z], e2[z] = hi, False
            else:
                if v <= l2[z]:
                    l1[z], n1[z], e1[z] = v, hi, True
                else:
                    l1[z], n1[z], e1[z] = l2[z], hi, False
                e2[z] = False
                if d2:
                    n2[z] = hi
            act = size != 0                                # the invariants the rules promise, for this v too
            act[z] = False
            act[lo] = False
            assert l1[z] <= D[z][act].min()
            if e1[z]:
                assert D[z, n1[z]] == l1[z] == D[z][act].min()
                rest = act.copy()
                rest[n1[z]] = False
                if rest.any():
                    assert l2[z] <= D[z][rest].min()
                    if e2[z]:
                        assert D[z, n2[z]] == l2[z] == D[z][rest].min()
        D[hi, lo] = D[lo, hi] = INF
        size[hi] = nlo + nhi
        cid[hi] = n + k
        m = size != 0
        m[hi] = False
        l1[hi], n1[hi], l2[hi], n2[hi] = top2_of(newrow, m)
        e1[hi], e2[hi] = n1[hi] >= 0, n2[hi] >= 0
        l1[lo] = INF
        k += 1
    return Z[:k], k, steps, rescans


def _masked_square(emb, group):
    from scipy.spatial.distance import pdist, squareform
    D = squareform(pdist(emb.astype(np.float64), "cosine"))
    D[group[:, None] == group[None, :]] = BIG
    np.fill_diagonal(D, np.inf)
    return D


@pytest.mark.parametrize("n,layout", [(2, "singletons"), (3, "singletons"), (23, "groups_3_4"), (60, "singletons"),
                                      (61, "groups_3_4"), (97, "huge_plus_singletons"), (40, "one_group"), (130, "groups_3_4")])
def test_step_rules_with_the_max_update_and_the_stop_equal_the_definition(n, layout):
    """The one claim the kernel change rests on: the I1 / I2 / e1 / e2 rules hold for v = max(d_xi, d_yi) (asserted after
    every update inside the model), the merge prefix equals scipy's on the masked matrix bit for bit (the model reads scipy's
    own distances), and stopping on a bound above the threshold — exact or stale — loses no merge."""
    emb, group = planted(n, 12, 7 + n), groups(layout, n)
    Z, allowed = definition(emb, group)
    D = _masked_square(emb, group)
    ts = [2.0, 1.0] + ([0.5 * allowed[0], float(np.median(allowed)), float(np.quantile(allowed, 0.1))] if len(allowed) else [])
    for t in ts:
        want = int(np.count_nonzero(Z[:, 2] <= t))
        got, m, steps, rescans = _link_top2_model(D, t)
        assert m == want, (t, m, want)
        assert np.array_equal(got, Z[:m]), t
        assert steps == m + rescans + (1 if m < n - 1 else 0)
    if layout == "one_group":
        assert int(np.count_nonzero(Z[:, 2] <= 2.0)) == 0 and (Z[:, 2] == BIG).all()


# ----------------------------------------------------------------------------- SpeakerLinker(backend="scipy")
DIM = 32


def _three_people(seed=3, noise=0.05):
    r = np.random.default_rng(seed)
    people = r.standard_normal((3, DIM))
    a = (people + noise * r.standard_normal((3, DIM))).astype(np.float32)
    b = (people + noise * r.standard_normal((3, DIM))).astype(np.float32)[[2, 0, 1]]      # b's label k is person (2, 0, 1)[k]
    return a, b


def _cos_dist(u, v):
    u, v = u.astype(np.float64), v.astype(np.float64)
    return 1.0 - float(u @ v) / float(np.linalg.norm(u) * np.linalg.norm(v))


def _link(threshold, adds, **kw):
    from diarizen_amd.linking import SpeakerLinker
    L = SpeakerLinker(threshold, dim=DIM, backend="scipy", **kw)
    for a in adds:
        L.add(*a)
    links = L.link()
    assert cannot_link_holds(links)
    assert L.device_calls == 0
    return links


def test_two_recordings_of_three_people_pair_the_right_labels():
    a, b = _three_people()
    links = _link(0.5, [("mon", a), ("tue", b)])
    assert links.num_identities == 3 and links.backend == "scipy" and links.unusable == []
    assert [links.identity[("mon", k)] for k in range(3)] == [0, 1, 2]                 # numbered by first appearance
    assert [links.identity[("tue", k)] for k in range(3)] == [2, 0, 1]
    assert links.members(2) == [("mon", 2), ("tue", 0)]
    assert links.names("tue") == {0: "spk0002", 1: "spk0000", 2: "spk0001"}
    assert links.names("tue", fmt="P{}") == {0: "P2", 1: "P0", 2: "P1"}


def test_threshold_1_9_still_gives_three_identities_only_because_of_the_constraint():
    """at 1.9 every cosine distance of this input is below the threshold: without the cannot-link mask everything collapses
    into one identity (checked), with it the three people stay apart"""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import pdist
    a, b = _three_people()
    y = pdist(np.concatenate([a, b]).astype(np.float64), "cosine")
    assert y.max() < 1.9 and len(set(fcluster(linkage(y, "complete"), 1.9, "distance"))) == 1
    links = _link(1.9, [("mon", a), ("tue", b)])
    assert links.num_identities == 3
    assert [links.identity[("tue", k)] for k in range(3)] == [2, 0, 1]


def test_threshold_below_every_distance_gives_singletons():
    a, b = _three_people()
    links = _link(1e-9, [("mon", a), ("tue", b)])
    assert links.num_identities == 6 and sorted(links.identity.values()) == list(range(6))
    assert all(v == 0.0 for v in links.diameter.values())


def test_numbering_is_invariant_under_row_permutations_inside_add_calls():
    a, b = _three_people()
    c = _three_people(seed=3, noise=0.04)[1]
    base = _link(0.5, [("mon", a), ("tue", b), ("wed", c)])
    r = np.random.default_rng(0)
    for _ in range(4):
        adds = []
        for name, rows in (("mon", a), ("tue", b), ("wed", c)):
            p = r.permutation(3)
            adds.append((name, rows[p], [int(k) for k in p]))            # row i carries label p[i]
        other = _link(0.5, adds)
        # the same partition; the numbers follow first appearance in add order, i.e. the row order of "mon" here
        part = lambda links: sorted(sorted(links.members(i)) for i in range(links.num_identities))
        assert part(other) == part(base)
        first = [other.identity[("mon", int(k))] for k in adds[0][2]]
        assert first == [0, 1, 2]


def test_diameter_is_the_largest_pairwise_distance_of_the_members():
    r = np.random.default_rng(20)
    people = r.standard_normal((7, DIM))                                 # six recordings, five of the seven people in each
    rows = {f"r{g}": (people[r.permutation(7)[:5]] + 0.3 * r.standard_normal((5, DIM))).astype(np.float32) for g in range(6)}
    links = _link(0.6, [(name, v) for name, v in rows.items()])
    assert 1 < links.num_identities < 30
    for i in range(links.num_identities):
        mem = links.members(i)
        pair = [_cos_dist(rows[ra][ka], rows[rb][kb]) for x, (ra, ka) in enumerate(mem) for (rb, kb) in mem[x + 1:]]
        want = max(pair) if pair else 0.0
        assert links.diameter[i] == pytest.approx(want, abs=1e-12) and links.diameter[i] <= 0.6
    assert any(len(links.members(i)) > 1 for i in range(links.num_identities))


def test_unusable_rows_empty_recordings_duplicate_names_and_relabel():
    from diarizen_amd.core import Annotation, Segment
    from diarizen_amd.linking import SpeakerLinker
    a, b = _three_people()
    bad = b.copy()
    bad[1] = 0.0                                                         # tue's label 1 (person 0) has no direction
    nan = a[:2].copy()
    nan[0, 3] = np.nan
    links = _link(0.5, [("mon", a), ("empty", np.zeros((0, DIM), np.float32)), ("tue", bad), ("wed", nan)])
    assert links.unusable == [("tue", 1), ("wed", 0)]
    assert links.identity[("tue", 0)] == links.identity[("mon", 2)] and links.identity[("tue", 2)] == links.identity[("mon", 1)]
    assert links.identity[("wed", 1)] == links.identity[("mon", 1)]
    own = [links.identity[k] for k in links.unusable]
    assert len(set(own)) == 2 and all(links.members(i) == [k] for i, k in zip(own, links.unusable))
    assert links.num_identities == 5 and links.names("empty") == {}
    # fewer than two usable rows: the trivial answer
    assert _link(0.5, []).num_identities == 0
    one = _link(0.5, [("x", a[:1]), ("y", np.zeros((2, DIM), np.float32))])
    assert one.backend == "trivial" and one.num_identities == 3 and len(one.unusable) == 2
    L = SpeakerLinker(0.5, dim=DIM, backend="scipy")
    L.add("mon", a)
    with pytest.raises(ValueError):
        L.add("mon", b)
    with pytest.raises(ValueError):
        L.add("tue", b, labels=[0, 0, 1])
    for t in (0.0, -1.0, 2.5, float("nan")):
        with pytest.raises(ValueError):
            SpeakerLinker(t)
    with pytest.raises(TypeError):
        SpeakerLinker()                                                  # no default threshold
    with pytest.raises(ValueError):
        SpeakerLinker(0.5, backend="cuda")
    # a live session is taken through its centroids
    live = type("Live", (), {"centroids": b})()
    L.add("live", live)
    assert L.link().identity[("live", 0)] == 2
    # relabel goes through identification.relabel: labels of the recording become the corpus-wide names
    ann = Annotation(uri="tue")
    ann[Segment(0.0, 1.0), "_"] = 0
    ann[Segment(1.0, 2.0), "_"] = 2
    ann[Segment(2.0, 3.0), "_"] = 7                                      # not a label of the linker: kept
    out = links.relabel("tue", ann)
    assert [lab for _, _, lab in out.itertracks(yield_label=True)] == ["spk0002", "spk0001", 7]
    assert out.uri == "tue"


def test_link_scipy_matches_the_case_generator_and_the_header_names_the_entry():
    from diarizen_amd import _lib
    from diarizen_amd.linking import link_scipy
    emb, group, Z, ts = case(65, 20, "groups_3_4")
    for t in ts:
        Zs, m = link_scipy(emb, group, t)
        assert np.array_equal(Zs, Z) and m == int(np.count_nonzero(Z[:, 2] <= t))
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dzn.h")).read()
    assert "int dzn_link_speakers(" in header and "dzn_link_speakers" in _lib.EXPORTED
