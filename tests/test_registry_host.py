"""The speaker registry on the host (diarizen_amd/registry.py, backend "numpy"; DiariZenPipeline.link_into) against the scipy
node-matrix definition: over the I + K nodes "identity i" and "new row k" the distances are BIG between two identities and
between two new rows and D[k, i] = max over the identity's rows of the float64 cosine distance otherwise;
linkage(condensed, "complete"), fcluster(Z, threshold, "distance"); row k joins identity i iff they share a flat cluster."""
import os

import numpy as np
import pytest

from _linking_cases import cannot_link_holds, distance_bound
from _registry_cases import (DIMS, NEW, STORED, assignment, case, columns, definition, greedy, seeded_registry)

DIM = 256


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", STORED)
def test_greedy_equals_the_scipy_definition_and_the_registry_runs_it(n, dim):
    for K in NEW:
        stored, ident, queries, D, ts = case(n, dim, K)          # (asserts the input condition)
        cols = columns(D)
        for t in ts:
            want = definition(D[:, cols], t)
            assert greedy(D[:, cols], t) == want, (K, t)
            reg, number = seeded_registry(stored, ident, t, "numpy", dim)
            before = reg.identity
            got = reg.add("new", queries)
            orig = assignment(D, t)                                  # {k: number in the case's `ident`}
            joined = {k: number[i] for k, i in orig.items()}
            fresh = iter(range(len(number), len(number) + K))
            assert got == {k: joined[k] if k in joined else next(fresh) for k in range(K)}, (K, t)
            assert reg.device_calls == 0 and reg.links().backend == "numpy"
            assert all(reg.identity[key] == i for key, i in before.items())
            for k, i in joined.items():                              # (the seeded diameters are 0)
                assert abs(reg.diameter[i] - D[k, orig[k]]) <= distance_bound(dim)
        if len(ts) == 3:
            assert definition(D[:, cols], ts[0]) == {}               # below the smallest entry nothing joins


def _pairwise_max(rows):
    from scipy.spatial.distance import pdist
    return float(pdist(rows.astype(np.float64), "cosine").max()) if len(rows) > 1 else 0.0


def _corpus(seed, people=12, noise=0.2, recordings=40, dim=DIM):
    """planted people, `recordings` recordings of 1-4 labels, no person twice in one -> [(name, rows, [person per label])]"""
    r = np.random.default_rng(seed)
    P = r.standard_normal((people, dim))
    out = []
    for j in range(recordings):
        who = r.choice(people, size=int(r.integers(1, 5)), replace=False)
        rows = (P[who] + noise * r.standard_normal((len(who), dim))).astype(np.float32)
        out.append((f"rec{j:02d}", rows, who.tolist()))
    return out


def _partition(identity):
    """{frozenset of keys}: the partition an identity dict stands for"""
    by = {}
    for key, i in identity.items():
        by.setdefault(i, set()).add(key)
    return {frozenset(v) for v in by.values()}


def test_guarantees_after_every_add_of_a_noisy_corpus():
    """diameter, cannot-link and stable numbers on a corpus whose people overlap (noise 0.6: wrong joins happen, the
    guarantees must hold anyway)"""
    from diarizen_amd.registry import SpeakerRegistry
    corpus = _corpus(3, people=8, noise=0.6, recordings=30, dim=32)
    t = 0.35
    reg = SpeakerRegistry(t, dim=32, backend="numpy")
    before, joins = {}, 0
    for name, rows, _ in corpus:
        got = reg.add(name, rows)
        now = reg.identity
        assert all(now[k] == i for k, i in before.items()) and len(now) == len(before) + len(rows)      # numbers are stable
        assert [now[(name, k)] for k in range(len(rows))] == [got[k] for k in range(len(rows))]
        joins += sum(i in set(before.values()) for i in got.values())
        before = now
        links = reg.links()
        assert cannot_link_holds(links) and links.num_identities == reg.num_identities == len(reg.diameter)
        ident = reg.row_identity
        for i, d in reg.diameter.items():
            assert _pairwise_max(reg.rows[ident == i]) <= d + distance_bound(32) and d <= t
    assert 0 < joins and reg.num_identities < len(reg)               # something joined, something did not
    assert len(reg) == sum(len(rows) for _, rows, _ in corpus)


def test_separated_corpus_gives_the_planted_people_in_every_order():
    from scipy.spatial.distance import cdist
    from diarizen_amd.linking import SpeakerLinker
    from diarizen_amd.registry import SpeakerRegistry
    corpus = _corpus(5)
    rows = np.concatenate([r for _, r, _ in corpus])
    who = np.concatenate([w for _, _, w in corpus])
    d = cdist(rows.astype(np.float64), rows.astype(np.float64), "cosine")
    same = who[:, None] == who[None, :]
    within, between = d[same].max(), d[~same].min()
    t = 0.4
    print(f"separated corpus: within-person max {within:.3f}, between-person min {between:.3f}, threshold {t}")
    assert within < t < between
    planted = {}
    for name, r, w in corpus:
        for k, p in enumerate(w):
            planted.setdefault(p, set()).add((name, k))
    planted = {frozenset(v) for v in planted.values()}
    L = SpeakerLinker(t, dim=DIM, backend="scipy")
    for name, r, _ in corpus:
        L.add(name, r)
    assert _partition(L.link().identity) == planted
    rng = np.random.default_rng(0)
    orders = [list(range(len(corpus))), list(range(len(corpus)))[::-1]] + [rng.permutation(len(corpus)).tolist() for _ in range(2)]
    for order in orders:
        reg = SpeakerRegistry(t, dim=DIM, backend="numpy")
        for j in order:
            reg.add(corpus[j][0], corpus[j][1])
        assert _partition(reg.identity) == planted and reg.num_identities == len(planted)
        assert all(v <= within + distance_bound(DIM) for v in reg.diameter.values())
        batch = reg.batch_links()
        assert batch.backend == "scipy" and _partition(batch.identity) == _partition(reg.links().identity)


def test_unusable_rows_empty_recordings_and_refusals():
    from diarizen_amd.registry import SpeakerRegistry
    (_, a, _), (_, b, _) = _corpus(7, people=4, recordings=2)[:2]
    a, b = np.concatenate([a, b])[:3], np.concatenate([a, b])[:3].copy()
    reg = SpeakerRegistry(0.4, dim=DIM, backend="numpy")
    assert reg.add("empty", np.zeros((0, DIM), np.float32)) == {} and len(reg) == 0 and reg.num_identities == 0
    assert reg.add("mon", a) == {0: 0, 1: 1, 2: 2}
    bad = b.copy()
    bad[1] = 0.0
    bad[2, 5] = np.nan
    got = reg.add("tue", bad, labels=["x", "y", "z"])
    assert got == {"x": 0, "y": 3, "z": 4} and reg.unusable == [("tue", "y"), ("tue", "z")]
    assert len(reg) == 4 and reg.num_identities == 5 and reg.diameter[3] == reg.diameter[4] == 0.0
    links = reg.links()
    assert links.unusable == reg.unusable and links.members(0) == [("mon", 0), ("tue", "x")] and links.members(3) == [("tue", "y")]
    assert links.names("tue") == {"x": "spk0000", "y": "spk0003", "z": "spk0004"} and links.names("empty") == {}
    # an unusable row is never matched against: the same zero row again founds another identity
    assert reg.add("wed", bad[1:2]) == {0: 5}
    state = (reg.identity, dict(reg.diameter), len(reg))
    with pytest.raises(ValueError):
        reg.add("mon", b)                                                # a recording name once
    with pytest.raises(ValueError):
        reg.add("thu", b, labels=[0, 0, 1])                              # distinct labels
    with pytest.raises(ValueError):
        reg.add("thu", b, labels=[0, 1])
    assert state == (reg.identity, dict(reg.diameter), len(reg))
    for t in (0.0, -1.0, 2.5, float("nan")):
        with pytest.raises(ValueError):
            SpeakerRegistry(t)
    with pytest.raises(TypeError):
        SpeakerRegistry()                                                # no default threshold
    with pytest.raises(ValueError):
        SpeakerRegistry(0.5, backend="scipy")
    with pytest.raises(ValueError):
        SpeakerRegistry(0.5, capacity=0)
    # a live session is taken through its centroids
    live = type("Live", (), {"centroids": a})()
    assert reg.add("live", live) == {0: 0, 1: 1, 2: 2}


def test_a_full_registry_refuses_and_changes_nothing():
    from diarizen_amd.registry import SpeakerRegistry
    corpus = _corpus(9, recordings=6)
    reg = SpeakerRegistry(0.4, dim=DIM, capacity=5, backend="numpy")
    stored = 0
    for name, rows, _ in corpus:
        if stored + len(rows) > 5:
            state = (reg.identity, dict(reg.diameter), len(reg), reg.rows.copy(), reg.unusable)
            with pytest.raises(MemoryError):
                reg.add(name, rows)
            assert state[:3] == (reg.identity, dict(reg.diameter), len(reg)) and np.array_equal(state[3], reg.rows)
            assert reg.add(name + "_unusable", np.zeros((2, DIM), np.float32)) != {}      # nothing to store: still fits
            break
        reg.add(name, rows)
        stored += len(rows)
    else:
        raise AssertionError("the corpus never filled the registry")


def _same_registry(a, b):
    assert a.identity == b.identity and a.diameter == b.diameter and a.unusable == b.unusable
    assert a.threshold == b.threshold and a.dim == b.dim and a.capacity == b.capacity and len(a) == len(b)
    assert np.array_equal(a.rows.view(np.uint32), b.rows.view(np.uint32)) and np.array_equal(a.row_identity, b.row_identity)
    la, lb = a.links(), b.links()
    assert all(la.members(i) == lb.members(i) for i in la.diameter)


def test_save_then_load_reproduces_every_field_and_the_next_add(tmp_path):
    from diarizen_amd.registry import SpeakerRegistry
    corpus = _corpus(11, recordings=12)
    reg = SpeakerRegistry(0.4, dim=DIM, capacity=100, backend="numpy")
    for name, rows, _ in corpus[:10]:
        reg.add(name, rows)
    reg.add("zero", np.zeros((1, DIM), np.float32), labels=["only"])
    path = tmp_path / "registry.npz"
    reg.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"rows", "ident", "threshold", "diameter", "meta"} and z["rows"].dtype == np.float32
    back = SpeakerRegistry.load(path)
    _same_registry(reg, back)
    assert back.backend == "numpy" and ("zero", "only") in back.unusable
    for name, rows, _ in corpus[10:]:
        assert reg.add(name, rows) == back.add(name, rows)
    _same_registry(reg, back)
    with pytest.raises(ValueError):
        back.add(corpus[0][0], corpus[0][1])                             # the names came back too
    odd = SpeakerRegistry(0.4, dim=DIM, backend="numpy")
    odd.add(("a", 1), corpus[0][1])
    with pytest.raises(ValueError):
        odd.save(tmp_path / "odd.npz")                                   # a tuple does not survive JSON


def test_from_links_then_add_equals_the_definition():
    from diarizen_amd.linking import SpeakerLinker
    from diarizen_amd.registry import SpeakerRegistry
    from _registry_cases import table
    corpus = _corpus(13, people=6, noise=0.5, recordings=20, dim=32)
    t = 0.45
    L = SpeakerLinker(t, dim=32, backend="scipy")
    for name, rows, _ in corpus[:15]:
        L.add(name, rows)
    L.add("none", np.zeros((1, 32), np.float32))
    links = L.link()
    reg = SpeakerRegistry.from_links(L, links, backend="numpy")
    assert reg.identity == links.identity and reg.diameter == links.diameter and reg.unusable == links.unusable
    assert reg.threshold == t and len(reg) == len(L) - 1
    for name, rows, _ in corpus[15:]:
        D = table(rows, reg.rows, reg.row_identity, reg.num_identities)
        want = assignment(D, t)
        n0 = reg.num_identities
        got = reg.add(name, rows)
        fresh = iter(range(n0, n0 + len(rows)))
        assert got == {k: want[k] if k in want else next(fresh) for k in range(len(rows))}
        assert cannot_link_holds(reg.links())


class _StubPipeline:
    """what link_into needs of a pipeline: diarize_many and rttm_out_dir"""

    def __init__(self, items, rttm_out_dir=None):
        self.items, self.rttm_out_dir, self.served = items, rttm_out_dir, 0

    def diarize_many(self, recordings, sess_names=None, return_embeddings=False):
        assert return_embeddings
        for rec, name in zip(recordings, sess_names):
            self.served += 1
            yield (name,) + self.items[rec]


def test_link_into_yields_each_recording_as_it_finishes(tmp_path):
    from diarizen_amd.core import Annotation, Segment
    from diarizen_amd.pipeline import DiariZenPipeline
    from diarizen_amd.registry import SpeakerRegistry
    corpus = _corpus(5, recordings=3)
    people = {}
    items = {}
    for name, rows, who in corpus:
        ann = Annotation(uri=name)
        for k in range(len(rows)):
            ann[Segment(float(k), float(k + 1)), "_"] = k
        items[name] = (ann, rows)
    stub = _StubPipeline(items, rttm_out_dir=str(tmp_path))
    reg = SpeakerRegistry(0.4, dim=DIM, backend="numpy")
    names = [c[0] for c in corpus]
    gen = DiariZenPipeline.link_into(stub, reg, names, sess_names=[n + "_s" for n in names], fmt="P{:02d}")
    for j, (name, rows, who) in enumerate(corpus):
        got_name, ann, ids = next(gen)
        assert stub.served == j + 1                                      # nothing waits for the end of the corpus
        assert got_name == name + "_s" and list(ids) == list(range(len(rows)))
        for k, p in enumerate(who):
            assert ids[k] == people.setdefault(p, ids[k])                # the planted people, whatever their numbers
        labels = [lab for _, _, lab in ann.itertracks(yield_label=True)]
        assert labels == [f"P{ids[k]:02d}" for k in range(len(rows))]
        assert (tmp_path / f"{name}_s.rttm").read_text() == ann.to_rttm()
        assert reg.identity[(name + "_s", 0)] == ids[0]
    with pytest.raises(StopIteration):
        next(gen)
    assert len(set(people.values())) == len(people)
    again = DiariZenPipeline.link_into(stub, reg, names[:1], sess_names=[names[0] + "_s"])
    with pytest.raises(ValueError):
        next(again)                                                      # a session name once
    assert stub.served == len(corpus) and names[0] + "_s" in reg and "other" not in reg      # refused before any device work
    twice = DiariZenPipeline.link_into(stub, reg, names[:2], sess_names=["x", "x"])
    with pytest.raises(ValueError):
        next(twice)
    none = DiariZenPipeline.link_into(stub, reg, names[:1], sess_names=[None])
    with pytest.raises(ValueError):
        next(none)


def test_the_header_names_the_entries():
    from diarizen_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dzn.h")).read()
    for name in ("dzn_registry_create", "dzn_registry_append", "dzn_registry_match", "dzn_registry_rows",
                 "dzn_registry_last_launch_ms", "dzn_registry_destroy"):
        assert f"int {name}(" in header and name in _lib.EXPORTED
