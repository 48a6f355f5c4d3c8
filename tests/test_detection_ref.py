"""Voice activity / overlapped speech detection on the host against tests/golden/detection_ref.npz, which
scripts/gen_detection_golden.py writes with the REFERENCE's own `Inference.aggregate` and `Binarize` (oracle/ref_host.py
imports them by path) and the two pipelines' pre-aggregation hooks (PA/pipelines/voice_activity_detection.py:125,
overlapped_speech_detection.py:132).  The product's numpy composition — postprocess.detection_scores_host (hook +
aggregate(hamming=True, missing=0.0) + crop) and binarize — must give every score bit and every RTTM byte.  When the
reference tree is present the recipe itself is re-run and compared with the committed file."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "detection_ref.npz"))
CASES = [str(c) for c in G["cases"]]
TASKS = {"speech": (1, "SPEECH"), "overlap": (2, "OVERLAP")}


def case_seg(name):
    src = str(G[f"{name}_src"])
    if src == "here":
        return G[f"{name}_seg"]
    f, key = src.split(":")
    return np.load(os.path.join(GOLD, f))[key]


def case_args(name):
    dur, ratio, n = G[f"{name}_args"]
    return float(dur), float(ratio), int(n)


def test_golden_covers_ties_crops_and_shapes():
    """what the fixture must contain to pin anything: exact 0.5 ties that keep their state, padded and unpadded last
    windows, S = 3 and 4, the 2241-window recording and the end-to-end decisions"""
    ties = sum(int(G[f"{n}_{t}_ties"]) for n in CASES for t in TASKS)
    assert ties >= 20
    assert {"host30", "EN2002a", "tie_w2s_c12"} <= set(CASES)
    from diarizen_amd.inference import window_plan
    padded = [window_plan(case_args(n)[2], int(case_args(n)[0] * 16000), int(round(case_args(n)[1] * case_args(n)[0] * 16000)))[1]
              for n in CASES]
    assert any(padded) and not all(padded)
    assert {case_seg(n).shape[2] for n in CASES} == {3, 4}


@pytest.mark.parametrize("task", list(TASKS))
@pytest.mark.parametrize("name", CASES)
def test_host_composition_equals_reference_run(name, task):
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import binarize, detection_scores_host, receptive_field
    bit, label = TASKS[task]
    dur, ratio, n = case_args(name)
    seg = case_seg(name)
    sc = detection_scores_host(seg, SlidingWindow(start=0.0, duration=dur, step=ratio * dur), receptive_field(), bit,
                               num_samples=n)
    ref = G[f"{name}_{task}_scores"]
    assert sc.data.dtype == np.float32 and sc.data.shape == ref.shape
    assert np.array_equal(sc.data.view(np.uint32), ref.view(np.uint32))
    ann = binarize(sc, onset=0.5, offset=0.5, uri=name)
    rttm = "".join(line.replace(" 0 <NA> <NA>\n", f" {label} <NA> <NA>\n") for line in ann.to_rttm().splitlines(True))
    assert rttm == G[f"{name}_{task}_rttm"].tobytes().decode()


@pytest.mark.parametrize("task", list(TASKS))
def test_activity_regions_and_hysteresis_equal_reference_run(task):
    """the split Binarize: per-frame activity (the golden's) -> regions with the pipeline label gives the RTTM; the
    activity is the hysteresis of the golden scores"""
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import _hysteresis, activity_regions
    _, label = TASKS[task]
    for name in CASES:
        sc, act = G[f"{name}_{task}_scores"][:, 0], G[f"{name}_{task}_active"]
        assert np.array_equal(_hysteresis(sc, 0.5, 0.5).astype(np.uint8), act)
        ann = activity_regions(act.astype(bool)[:, None], SlidingWindow(start=0.0, duration=0.025, step=0.02), uri=name,
                               labels=[label])
        assert ann.to_rttm() == G[f"{name}_{task}_rttm"].tobytes().decode()


def test_overlap_frames_are_speech_frames():
    for name in CASES:
        assert not np.any(G[f"{name}_overlap_active"].astype(bool) & ~G[f"{name}_speech_active"].astype(bool)), name


def test_annotation_support_follows_pyannote_core():
    """Annotation.support(collar) (min_duration_off of Binarize): per label, gaps shorter than the collar (or empty) are
    filled; touching and overlapping segments merge; other labels stay apart"""
    from diarizen_amd.core import Annotation, Segment
    a = Annotation(uri="u")
    for s, e, lab in ((0.0, 1.0, "S"), (1.2, 2.0, "S"), (2.0, 2.5, "S"), (3.0, 4.0, "S"), (3.5, 3.7, "S"),
                      (0.5, 0.7, "O"), (0.9, 1.0, "O")):
        a[Segment(s, e), len(list(a.itertracks()))] = lab
    got = [(seg.start, seg.end, lab) for seg, _, lab in a.support(collar=0.3).itertracks(yield_label=True)]
    assert got == [(0.0, 2.5, "S"), (0.5, 1.0, "O"), (3.0, 4.0, "S")]
    got0 = [(seg.start, seg.end) for seg, _, lab in a.support().itertracks(yield_label=True) if lab == "S"]
    assert got0 == [(0.0, 1.0), (1.2, 2.5), (3.0, 4.0)]
    b = a.support(0.3)
    seg, tr = next(iter(b.itertracks()))
    del b[seg, tr]
    assert len(list(b.itertracks())) == 2


def _reference_available():
    from oracle import ref_host
    return ref_host.available()


@pytest.mark.skipif(not _reference_available(), reason="needs the reference tree (build container only)")
def test_reference_functions_reproduce_committed_golden():
    """the recipe of scripts/gen_detection_golden.py on every case (the end-to-end case from its committed decisions; their
    forward is the oracle's, pinned to the reference modules by tests/test_oracle.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "gen_detection_golden", os.path.join(os.path.dirname(__file__), "..", "scripts", "gen_detection_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = {c[0]: c for c in gen.load_cases(e2e=False)}
    for name in CASES:
        seg = case_seg(name)
        if name in cases:
            assert np.array_equal(cases[name][1], seg)
            assert np.array_equal(np.array(cases[name][2:5], dtype=np.float64), G[f"{name}_args"])
        dur, ratio, n = case_args(name)
        for task in TASKS:
            sc, act, rttm = gen.reference_detection(seg, dur, ratio, n, task, name)
            assert np.array_equal(sc.view(np.uint32), G[f"{name}_{task}_scores"].view(np.uint32))
            assert np.array_equal(act, G[f"{name}_{task}_active"])
            assert rttm == G[f"{name}_{task}_rttm"].tobytes().decode()
