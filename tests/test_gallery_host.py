"""Speaker identification, the parts that need no GPU (diarizen_amd/identification.py, the centroids of
pipeline.run_host_stage): the library exports the gallery ABI, assign_identities against brute force, the SpeakerGallery
bookkeeping, relabel, and the host stage handing the clustering's centroids out."""
import os

import numpy as np
import pytest

from _gallery_cases import assignment_case, brute_force_objective, objective

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_gallery_symbols_are_exported(built_lib):
    from diarizen_amd import _lib
    names = ["dzn_gallery_create", "dzn_gallery_put", "dzn_gallery_drop", "dzn_gallery_search", "dzn_gallery_geometry",
             "dzn_gallery_rows", "dzn_gallery_last_launch_ms", "dzn_gallery_destroy"]
    for n in names:
        assert n in _lib.EXPORTED and hasattr(built_lib, n), n
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dzn.h")).read()
    assert all(f"int {n}(" in header for n in names) and "No reference counterpart" in header


# ----------------------------------------------------------------------------- assign_identities
ASSIGN = [(seed, K, n) for seed, (K, n) in enumerate([(1, 1), (1, 4), (2, 2), (2, 5), (3, 3), (3, 6), (4, 4), (4, 6), (4, 2)])]


@pytest.mark.parametrize("seed,K,n", ASSIGN)
@pytest.mark.parametrize("threshold", [0.0, 0.3, 0.5, 0.7, 1.0])       # below, between and above the scores (0.05 .. 0.95)
def test_assign_identities_equals_brute_force(seed, K, n, threshold):
    from diarizen_amd.identification import assign_identities
    scores, slots = assignment_case(seed, K, n)
    matched = assign_identities(scores, slots, threshold)
    assert len(matched) == K
    used = [m for m in matched if m is not None]
    assert len(used) == len(set(used))                                  # never a name twice
    got, best = objective(scores, slots, threshold, matched), brute_force_objective(scores, slots, threshold)
    assert got == pytest.approx(best, abs=1e-12)
    if threshold >= 1.0:
        assert used == []
    if threshold <= 0.0:
        assert len(used) == min(K, n)


def test_assign_identities_is_exclusive_where_a_greedy_rule_is_not():
    from diarizen_amd.identification import assign_identities
    # both labels like slot 7 best; label 1 likes it more, label 0 has a second choice above the threshold
    scores = np.array([[0.90, 0.80], [0.95, 0.10]])
    slots = np.array([[7, 3], [7, 3]])
    assert assign_identities(scores, slots, 0.5) == [3, 7]
    assert assign_identities(scores, slots, 0.85) == [None, 7]          # 0.95 - 0.85 beats 0.90 - 0.85
    assert assign_identities(scores, slots, 0.99) == [None, None]
    assert assign_identities(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), 0.5) == []
    # empty candidates (slot -1, score -inf) are never matched
    assert assign_identities(np.array([[0.9, -np.inf]]), np.array([[4, -1]]), 0.5) == [4]
    assert assign_identities(np.array([[-np.inf, -np.inf]]), np.array([[-1, -1]]), -1.0) == [None]


@pytest.mark.parametrize("seed,K,n", [(11, 2, 6), (12, 3, 6), (13, 4, 6), (14, 4, 5)])
@pytest.mark.parametrize("threshold", [0.2, 0.5, 0.8])
def test_assign_identities_on_top_k_lists_equals_dense_lists(seed, K, n, threshold):
    """with n >= K candidates per label the restriction to the per-label top K loses nothing (exchange argument)"""
    from diarizen_amd.identification import assign_identities
    scores, slots = assignment_case(seed, K, n)
    dense = assign_identities(scores, slots, threshold)
    top = assign_identities(scores[:, :K], slots[:, :K], threshold)
    assert objective(scores, slots, threshold, top) == pytest.approx(objective(scores, slots, threshold, dense), abs=1e-12)
    assert objective(scores, slots, threshold, dense) == pytest.approx(brute_force_objective(scores, slots, threshold), abs=1e-12)


# ----------------------------------------------------------------------------- SpeakerGallery bookkeeping
def _prints(n, dim=32, seed=0):
    return np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)


def test_gallery_bookkeeping_replace_reuse_growth():
    from diarizen_amd.identification import SpeakerGallery
    v = _prints(12)
    g = SpeakerGallery(dim=32, capacity=4)
    assert len(g) == 0 and g.names == [] and "ann" not in g
    assert [g.enroll(n, v[i]) for i, n in enumerate(["ann", "bob", "cy"])] == [0, 1, 2]
    assert g.enroll("bob", v[5]) == 1 and len(g) == 3                   # re-enrolling replaces the row
    assert np.array_equal(g.voiceprint("bob"), v[5]) and g.names == ["ann", "bob", "cy"]
    g.remove("ann")
    assert "ann" not in g and len(g) == 2 and g.names == ["bob", "cy"]
    with pytest.raises(KeyError):
        g.remove("ann")
    assert g.enroll("dee", v[6]) == 0                                   # the freed slot is reused
    assert g.names == ["dee", "bob", "cy"]
    assert g.capacity == 4
    for i in range(7, 12):
        g.enroll(f"p{i}", v[i])                                         # past the capacity: doubled
    assert g.capacity == 8 and len(g) == 8 and g.slot_of("p11") == 7
    g.enroll("q", v[0])
    assert g.capacity == 16 and np.array_equal(g.voiceprint("cy"), v[2])
    assert g.searches == 0                                              # nothing above touched a device


def test_gallery_refuses_bad_names_and_voiceprints():
    from diarizen_amd.identification import SpeakerGallery
    g = SpeakerGallery(dim=32)
    v = _prints(1)[0]
    for name in ("", "two words", "tab\tbed", "line\n", None, 3):
        with pytest.raises(ValueError):
            g.enroll(name, v)
    for bad in (np.zeros(32, np.float32), np.where(np.arange(32) == 3, np.nan, v), np.where(np.arange(32) == 0, np.inf, v),
                v[:16]):
        with pytest.raises(ValueError):
            g.enroll("ok", bad)
    assert len(g) == 0
    for dim in (8, 24, 528):
        with pytest.raises(ValueError):
            SpeakerGallery(dim=dim)


def test_gallery_save_load_round_trip(tmp_path):
    from diarizen_amd.identification import SpeakerGallery
    v = _prints(6)
    g = SpeakerGallery(dim=32, capacity=4)
    for i, n in enumerate(["zoe", "ann", "bob", "cy", "dee", "eve"]):
        g.enroll(n, v[i])
    g.remove("bob")
    path = tmp_path / "people.gallery"                                  # (no .npz appended)
    g.save(path)
    assert path.exists()
    h = SpeakerGallery.load(path)
    assert h.names == g.names == ["zoe", "ann", "cy", "dee", "eve"] and h.dim == 32
    for n in g.names:
        assert np.array_equal(h.voiceprint(n).view(np.uint32), g.voiceprint(n).view(np.uint32))
    with np.load(path, allow_pickle=False) as z:
        assert z["voiceprints"].dtype == np.float32 and z["voiceprints"].shape == (5, 32) and z["names"].dtype.kind == "U"
    empty = tmp_path / "none.npz"
    SpeakerGallery(dim=32).save(empty)
    assert SpeakerGallery.load(empty).names == []


# ----------------------------------------------------------------------------- relabel, centroids
def test_relabel_substitutes_the_label_column_of_the_rttm():
    from diarizen_amd.core import Annotation, Segment
    from diarizen_amd.identification import relabel
    ann = Annotation(uri="call7")
    for i, (a, b, lab) in enumerate([(0.0, 1.5, 0), (1.0, 2.25, 1), (2.5, 3.0, 0), (3.0, 4.125, 2), (3.5, 3.75, 1)]):
        ann[Segment(a, b), i] = lab
    names = {0: "agent_ann", 2: "customer_17"}
    out = relabel(ann, names)
    expect = []
    for line in ann.to_rttm().splitlines():
        f = line.split(" ")
        f[7] = str(names.get(int(f[7]), f[7]))
        expect.append(" ".join(f))
    assert out.to_rttm().splitlines() == expect and out.uri == "call7"
    assert set(map(str, out.labels())) == {"1", "agent_ann", "customer_17"}             # the unmatched label is kept
    assert relabel(ann, {}).to_rttm() == ann.to_rttm()


def test_run_host_stage_hands_the_clusterings_centroids_out_unchanged():
    from diarizen_amd.clustering import AgglomerativeClustering
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.pipeline import run_host_stage
    from oracle.gen_golden import E2E_CONFIG
    g = np.load(os.path.join(GOLD, "e2e_EN2002a_30s.npz"))
    rttm = open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read()
    clu = E2E_CONFIG["clustering"]["args"]
    ahc = AgglomerativeClustering(metric="cosine", method="centroid", min_cluster_size=clu["min_cluster_size"],
                                  threshold=clu["ahc_threshold"])
    hard, _, centroids = ahc(embeddings=g["emb"], segmentations=g["seg"].astype(np.float32), min_clusters=1, max_clusters=20)
    seen = {}
    kw = dict(chunks=SlidingWindow(start=0.0, duration=8.0, step=0.8), clustering=ahc, min_speakers=clu["min_speakers"],
              max_speakers=clu["max_speakers"], sess_name="EN2002a")
    ann, emb = run_host_stage(g["seg"], g["emb"], hook=lambda name, artifact, **k: seen.setdefault(name, artifact),
                              return_embeddings=True, **kw)
    assert list(seen) == ["speaker_counting", "centroids", "discrete_diarization"]
    assert seen["centroids"].dtype == centroids.dtype and np.array_equal(seen["centroids"], centroids)
    K = int(hard.max()) + 1
    assert emb.dtype == np.float32 and emb.shape == (K, 256) and np.array_equal(emb, centroids.astype(np.float32))
    assert ann.to_rttm() == rttm                                        # the annotation of a call without the flag
    assert run_host_stage(g["seg"], g["emb"], **kw).to_rttm() == rttm   # ... which still returns the Annotation alone


def test_voiceprint_takes_the_dominant_label_and_refuses_a_recording_without_speech():
    """DiariZenPipeline.voiceprint over a stand-in for the call it makes: the largest total duration wins, ties go to the
    smaller label, no speech is a ValueError"""
    from diarizen_amd.core import Annotation, Segment
    from diarizen_amd.pipeline import DiariZenPipeline
    emb = np.arange(3 * 256, dtype=np.float32).reshape(3, 256)

    class Call:
        def __init__(self, turns):
            self.ann = Annotation(uri="x")
            for i, (a, b, lab) in enumerate(turns):
                self.ann[Segment(a, b), i] = lab

        def __call__(self, wav, sess_name=None, return_embeddings=False):
            assert return_embeddings
            return self.ann, emb

    v = DiariZenPipeline.voiceprint(Call([(0.0, 1.0, 0), (1.0, 2.5, 2), (3.0, 4.0, 0), (4.0, 4.25, 1)]), None)
    assert v.dtype == np.float32 and np.array_equal(v, emb[0]) and v is not emb[0]
    assert np.array_equal(DiariZenPipeline.voiceprint(Call([(0.0, 1.0, 2), (1.0, 2.0, 1)]), None), emb[1])      # a tie
    with pytest.raises(ValueError):
        DiariZenPipeline.voiceprint(Call([]), None)
