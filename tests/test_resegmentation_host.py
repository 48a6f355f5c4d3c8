"""Resegmentation without a device: the pure functions of diarizen_amd/postprocess.py (hypothesis on the frame grid, trim and
row arithmetic, the numpy twin of dzn_match_counts) on known answers, and the host composition (postprocess.resegment_host +
resegmentation.annotation_from_discrete) against every case of tests/golden/resegmentation_ref.npz
(scripts/gen_resegmentation_golden.py: the reference's own speaker_count / trim / permutate / to_diarization / Binarize)."""
import numpy as np
import pytest

from _reseg_cases import CASES, G, case_inputs, check_against_golden


def test_golden_has_every_kind_of_hypothesis():
    kinds = {c.rsplit("_", 2)[-2] for c in CASES}
    assert kinds == {"perm", "later", "earlier", "k2", "k6", "empty", "ghost"}
    assert {c.rsplit("_", 1)[-1] for c in CASES} == {"w00", "w05"}
    assert any(G[f"{c}_ref"].shape[1] > G[f"{c}_hard"].shape[1] for c in CASES)         # K > S: the decisions are widened
    assert any(0 < G[f"{c}_ref"].shape[1] < G[f"{c}_hard"].shape[1] for c in CASES)     # K < S: the hypothesis is widened
    assert max(len(G[f"{c}_hard"]) for c in CASES) > 2000


def test_discretize_turns_known_answers():
    """frame i of the receptive field is centred at 0.02 i + 0.00496875 s: closest_frame(t) = rint((t - 0.00496875) / 0.02)"""
    from diarizen_amd.postprocess import discretize_turns, receptive_field
    fr = receptive_field()
    # a turn ending exactly on the centre of frame 20 includes it (SlidingWindow.crop(mode="center"): both ends closest_frame)
    ref, labels = discretize_turns([(0.1, 0.40496875, "a")], fr, 30)
    assert labels == ["a"] and ref.dtype == np.uint8 and ref.shape == (30, 1)
    assert np.array_equal(np.nonzero(ref[:, 0])[0], np.arange(5, 21))
    # beyond Tr: clipped to the last row; wholly beyond: nothing; ending before 0: outside the support
    ref, _ = discretize_turns([(0.5, 2.0, "a"), (1.0, 2.0, "b"), (-1.0, -0.001, "c"), (-1.0, 0.05, "d")], fr, 30)
    assert np.array_equal(np.nonzero(ref[:, 0])[0], np.arange(25, 30))
    assert not ref[:, 1].any() and not ref[:, 2].any()
    assert np.array_equal(np.nonzero(ref[:, 3])[0], np.arange(0, 3))            # closest_frame(0.05) = rint(2.25) = 2
    # overlapping turns of one label are one run of ones
    ref, _ = discretize_turns([(0.1, 0.3, "a"), (0.2, 0.4, "a")], fr, 30)
    assert np.array_equal(np.nonzero(ref[:, 0])[0], np.arange(5, 21)) and ref.max() == 1
    # labels sorted by str(): 10 < 9 < b
    ref, labels = discretize_turns([(0.0, 0.1, 9), (0.2, 0.3, "b"), (0.4, 0.5, 10)], fr, 30)
    assert labels == [10, 9, "b"]
    assert [int(np.nonzero(ref[:, k])[0][0]) for k in range(3)] == [20, 0, 10]
    # an Annotation is read through itertracks
    from diarizen_amd.core import Annotation, Segment
    ann = Annotation()
    ann[Segment(0.1, 0.3), "x"] = "a"
    ann[Segment(0.2, 0.4), "y"] = "a"
    assert np.array_equal(discretize_turns(ann, fr, 30)[0], discretize_turns([(0.1, 0.3, "a"), (0.2, 0.4, "a")], fr, 30)[0])
    assert discretize_turns([], fr, 30)[0].shape == (30, 0) and discretize_turns([], fr, 0)[0].shape == (0, 0)


@pytest.mark.parametrize("duration,L,expect", [
    (8.0, 399, {0.0: (0, 399, [0, 40, 80]), 0.05: (20, 359, [20, 60, 100]), 0.1: (40, 319, [40, 80, 120])}),
    (16.0, 799, {0.0: (0, 799, [0, 80, 160]), 0.05: (40, 719, [40, 120, 200]), 0.1: (80, 639, [80, 160, 240])}),
])
def test_trim_and_first_reference_row(duration, L, expect):
    """l0 = round(L w), L' = L - 2 l0 (Inference.trim); r_c = max(0, ceil((c step + w D - 0.025 + 0.00753125) / 0.02)), the
    loose crop of the trimmed chunk on the receptive field"""
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import receptive_field, reference_rows, trim_frames, trimmed_chunks
    chunks = SlidingWindow(start=0.0, duration=duration, step=0.1 * duration)
    for w, (l0, Lt, rows) in expect.items():
        assert trim_frames(L, w) == (l0, Lt)
        tc = trimmed_chunks(chunks, w)
        assert tc.step == chunks.step and abs(tc.start - w * duration) < 1e-12 and abs(tc.duration - (1 - 2 * w) * duration) < 1e-12
        r = reference_rows(3, tc, receptive_field())
        assert r.dtype == np.int32 and r.tolist() == rows


def test_reference_extent():
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import receptive_field, reference_extent
    chunks = SlidingWindow(start=0.0, duration=8.0, step=0.8)
    assert reference_extent(128000, 16000, chunks, receptive_field()) == (0, 440)       # closest_frame(8.8) = rint(439.75)


@pytest.mark.parametrize("C,L,S,K,l0,Lt", [(3, 7, 4, 1, 0, 7), (2, 65, 4, 5, 3, 59), (1, 1, 4, 0, 0, 1), (2, 70, 3, 2, 3, 64),
                                            (2, 9, 2, 33, 1, 7)])
def test_match_counts_host_equals_triple_loop(C, L, S, K, l0, Lt):
    from diarizen_amd.postprocess import match_counts_host
    g = np.random.default_rng(C * 1000 + L)
    seg = (g.random((C, L, S)) < 0.4).astype(np.uint8)
    Tr = L + 3
    ref = (g.random((Tr, K)) < 0.5).astype(np.uint8)
    rows = np.array([0, 5, Tr - 2][:C], dtype=np.int32)                 # the last window runs past Tr
    got = match_counts_host(seg, ref, rows, l0, Lt, K)
    n = max(K, S)
    assert got.shape == (C, n, n) and got.dtype == np.int32
    for c in range(C):
        for i in range(n):
            for j in range(n):
                d = 0
                for l in range(Lt):
                    r = rows[c] + l
                    a = int(ref[r, i]) if i < K and r < Tr else 0
                    b = int(seg[c, l0 + l, j]) if j < S else 0
                    d += a != b
                assert got[c, i, j] == d, (c, i, j)
    with pytest.raises(ValueError):
        match_counts_host(seg, ref, rows, l0, L - l0 + 1, K)


@pytest.mark.parametrize("name", CASES)
def test_host_composition_equals_reference_run(name):
    """hypothesis text -> matrix -> counts -> assignment -> count -> discrete diarization -> RTTM: every array and every
    byte of the reference's run"""
    from diarizen_amd.postprocess import discretize_turns, receptive_field, reference_extent, resegment_host
    seg, turns, chunks, w, num_samples = case_inputs(name)
    frames = receptive_field()
    _, Tr = reference_extent(num_samples, 16000, chunks, frames)
    ref, labels = discretize_turns(turns, frames, Tr)
    assert np.array_equal(ref, G[f"{name}_ref"]) and [str(x) for x in labels] == [str(x) for x in G[f"{name}_labels"]]
    count, counts, hard, discrete = resegment_host(seg, ref, chunks, frames, w)
    assert hard.shape == seg.shape[::2] and hard.dtype == np.int8
    assert all(len(set(row)) == len(row) for row in hard.tolist())              # a window's local speakers go to distinct columns
    check_against_golden(name, seg, chunks, w, count, counts, hard, discrete)


def test_onset_and_offset_are_refused_by_name():
    from diarizen_amd.resegmentation import Resegmentation
    r = Resegmentation.__new__(Resegmentation)
    for bad in ({"onset": 0.5}, {"offset": 0.5}, {"warm_up": 0.0, "onset": 0.8}):
        with pytest.raises(ValueError, match="onset"):
            r.instantiate(bad)
    assert r.default_parameters() == {"warm_up": 0.0, "min_duration_on": 0.0, "min_duration_off": 0.0}


def test_hypothesis_forms(tmp_path):
    """an Annotation, RTTM text, a path, a list of turns; an empty one is K = 0, a missing one an error"""
    from diarizen_amd.core import Annotation, Segment
    from diarizen_amd.postprocess import discretize_turns, receptive_field
    from diarizen_amd.resegmentation import as_hypothesis
    text = ("SPEAKER rec 1 0.100 0.200 <NA> <NA> b <NA> <NA>\nSPEAKER other 1 0.000 9.000 <NA> <NA> z <NA> <NA>\n"
            "SPEAKER rec 1 0.200 0.200 <NA> <NA> a <NA> <NA>\n")
    p = tmp_path / "rec.rttm"
    p.write_text(text)
    ann = Annotation(uri="rec")
    ann[Segment(0.1, 0.1 + 0.2), 0] = "b"
    ann[Segment(0.2, 0.4), 1] = "a"
    fr = receptive_field()
    want, labels = discretize_turns(ann, fr, 40)
    assert labels == ["a", "b"]
    for form in (text, str(p), p, as_hypothesis(text, "rec")):
        ref, lab = discretize_turns(as_hypothesis(form, "rec"), fr, 40)
        assert lab == labels and np.array_equal(ref, want)
    assert discretize_turns(as_hypothesis(text, "unknown"), fr, 40)[1] == ["a", "b", "z"]       # no line names the uri: all lines
    for empty in ("", Annotation(), []):
        ref, lab = discretize_turns(as_hypothesis(empty, "rec"), fr, 40)
        assert ref.shape == (40, 0) and lab == []
    with pytest.raises(ValueError, match="diarization"):
        as_hypothesis(None)


def test_empty_hypothesis_is_four_new_speakers():
    """K = 0: every column is one the hypothesis did not have; the speaker count and therefore the number of active speakers
    per frame are the decisions' own"""
    from diarizen_amd.postprocess import receptive_field, resegment_host
    seg, _, chunks, w, _ = case_inputs("EN2002a_empty_w00")
    count, counts, hard, discrete = resegment_host(seg, np.zeros((100, 0), np.uint8), chunks, receptive_field(), w)
    assert counts.shape[1:] == (4, 4) and np.array_equal(counts, np.broadcast_to(seg.sum(axis=1, dtype=np.int32)[:, None, :],
                                                                                  counts.shape))
    assert discrete.data.shape[1] == 4
    assert np.array_equal(discrete.data.sum(axis=1), count.data[:, 0])


def test_relabelling_through_labels():
    """the result's integer labels are columns of the sorted hypothesis labels: identification.relabel puts the names back; a
    hypothesis whose names sort differently gives the same speakers under those names wherever the top-count selection has no
    tie to break by column order"""
    from diarizen_amd.identification import relabel
    from diarizen_amd.postprocess import receptive_field, resegment_host
    from diarizen_amd.resegmentation import annotation_from_discrete
    from _reseg_cases import renamed_runs_agree
    seg, turns, chunks, w, num_samples = case_inputs("EN2002a_perm_w00")
    rename = {"spk00": "carol", "spk01": "alice", "spk02": "bob"}
    runs = []

    def run(ref):
        runs.append(resegment_host(seg, ref, chunks, receptive_field(), w))
        return runs[-1]
    old, new = renamed_runs_agree(seg, turns, rename, chunks, num_samples, run)
    assert old == ["spk00", "spk01", "spk02"] and new == ["alice", "bob", "carol"]
    ann = annotation_from_discrete(runs[0][3], uri="EN2002a")
    # (column 3 is a speaker the three-speaker hypothesis did not have: it keeps its integer label)
    assert ann.labels() == [0, 1, 2, 3]
    named = relabel(ann, dict(enumerate(old)))
    assert named.labels() == [3, "spk00", "spk01", "spk02"]
    assert [(s, t) for s, t, _ in named.itertracks(yield_label=True)] == [(s, t) for s, t, _ in ann.itertracks(yield_label=True)]
