"""Per-speaker activity scores on the host against tests/golden/scores_ref.npz, which scripts/gen_scores_golden.py writes
with the REFERENCE's own `Powerset.to_multilabel(soft=True)`, `SpeakerDiarization.reconstruct` (its clustered scores) and
`Inference.aggregate(hamming=True, missing=0.0, warm_up)` (oracle/ref_host.py imports them by path).  The product's numpy
restatement — postprocess.speaker_scores — must give every score bit, the cropped and the warm-up case included;
postprocess.soft_multilabel must give the reference's soft multilabel scores to float32 rounding.  When the reference tree is
present the recipe itself is re-run and compared with the committed file."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "scores_ref.npz"))
AGG = [str(c) for c in G["agg_cases"]]
ML = [str(c) for c in G["ml_cases"]]
SR = 16000


def case(name):
    """-> (soft, hard, chunks, warm_up, number of frames the golden keeps)"""
    from diarizen_amd.core import SlidingWindow
    dur, ratio, n, w0, w1 = (float(v) for v in G[f"{name}_args"])
    return (G[f"{name}_soft"], G[f"{name}_hard"], SlidingWindow(start=0.0, duration=dur, step=ratio * dur), (w0, w1),
            len(G[f"{name}_scores"]))


def test_golden_covers_the_cases_that_pin_the_arithmetic():
    """-2 entries, a cluster absent from some windows, a cluster absent from every window that covers some frame (its score
    there is exactly 0.0 while others live), two local speakers of one window in one cluster; C = 1, K = 1, K = 32, a
    ten-windows-deep case, a cropped case and a warm-up case"""
    from diarizen_amd.inference import window_plan
    from diarizen_amd.postprocess import _frame_grid, receptive_field
    hards = [G[f"{n}_hard"] for n in AGG]
    assert any((h == -2).any() for h in hards)
    assert any(not (row == k).any() for h in hards for row in h for k in range(int(h.max()) + 1))
    assert any(len(set(row[row >= 0].tolist())) < int((row >= 0).sum()) for h in hards for row in h)
    sc = G["w2s_c12_s4_k5_scores"]
    assert np.all(sc[200:249, 0] == 0.0) and np.all(sc[200:249, 1:].max(axis=1) > 0.0)
    shapes = {n: (G[f"{n}_soft"].shape, G[f"{n}_scores"].shape[1]) for n in AGG}
    assert ((12, 99, 4), 5) in shapes.values() and ((23, 99, 3), 2) in shapes.values()
    assert any(s[0][0] == 1 for s in shapes.values()) and {1, 32} <= {s[1] for s in shapes.values()}
    cropped, warm = [], []
    for n in AGG:
        soft, hard, chunks, warm_up, T = case(n)
        full = _frame_grid(soft.shape[0], soft.shape[1], chunks, receptive_field())[2]
        padded = window_plan(int(G[f"{n}_args"][2]), int(chunks.duration * SR), int(round(chunks.step * SR)))[1]
        assert (T < full) == padded
        cropped.append(T < full)
        warm.append(warm_up != (0.0, 0.0))
    assert any(cropped) and not all(cropped) and any(warm)
    # the deep case's window starts are not multiples of the frame step in float64: closest_frame has to round
    _, _, chunks, _, _ = case("w2s_c23_s3_k2_deep")
    assert any((c * chunks.step / 0.02) != round(c * chunks.step / 0.02) for c in range(23))
    assert os.path.getsize(os.path.join(GOLD, "scores_ref.npz")) <= os.path.getsize(os.path.join(GOLD, "detection_ref.npz"))


@pytest.mark.parametrize("name", AGG)
def test_host_speaker_scores_equal_reference_run(name):
    from diarizen_amd.postprocess import crop_end, receptive_field, speaker_scores
    soft, hard, chunks, warm_up, T = case(name)
    got = speaker_scores(soft, chunks, receptive_field(), hard, warm_up=warm_up)
    ref = G[f"{name}_scores"]
    grid = got.sliding_window
    assert grid.start == 0.0 and grid.step == 0.02 and grid.duration == 0.025
    assert got.data.dtype == np.float32 and got.data.shape[1] == ref.shape[1]
    n = int(G[f"{name}_args"][2])
    keep = crop_end(len(got.data), grid, n / SR) if T < len(got.data) else len(got.data)
    assert keep == T
    assert np.array_equal(got.data[:keep].view(np.uint32), ref.view(np.uint32))


def test_warm_up_tables_matter():
    """the warm-up case is not the (0, 0) aggregate; with hamming alone speaker_scores is aggregate() on the clustered scores"""
    from diarizen_amd.postprocess import aggregate, clustered_scores, receptive_field, speaker_scores
    name = "w2s_c12_warm_up"
    soft, hard, chunks, warm_up, T = case(name)
    ref = G[f"{name}_scores"]
    plain = speaker_scores(soft, chunks, receptive_field(), hard).data[:T]
    assert not np.array_equal(plain, ref)
    one = aggregate(clustered_scores(soft, hard), chunks, receptive_field(), hamming=True, missing=0.0).data[:T]
    assert np.array_equal(one.view(np.uint32), plain.view(np.uint32))


def test_no_cluster_gives_zero_columns():
    from diarizen_amd.postprocess import _frame_grid, receptive_field, speaker_scores
    soft, hard, chunks, _, _ = case("w2s_c7_padded")
    got = speaker_scores(soft, chunks, receptive_field(), np.full_like(hard, -2))
    full = _frame_grid(soft.shape[0], soft.shape[1], chunks, receptive_field())[2]
    assert got.data.shape == (full, 0) and got.data.dtype == np.float32


@pytest.mark.parametrize("name", ML)
def test_soft_multilabel_agrees_with_reference_powerset(name):
    """exp(logp) @ mapping in float32: at most 7 of the 11 classes contain a speaker, each term in [0, 1] with a few ulp of
    exp and float32 summation in whatever order the two matmuls take -> 1e-6"""
    from diarizen_amd.postprocess import soft_multilabel
    logp = np.load(os.path.join(GOLD, f"{name}.npz"))["logp"]
    ref = G[f"{name}_soft"]
    got = soft_multilabel(logp, G["mapping_4_2"])
    assert got.dtype == np.float32 and got.shape == ref.shape == logp.shape[:-1] + (4,)
    assert float(np.abs(got - ref).max()) <= 1e-6
    assert float(ref.min()) >= 0.0 and float(ref.max()) <= 1.0 + 1e-6


def _reference_available():
    from oracle import ref_host
    return ref_host.available()


@pytest.mark.skipif(not _reference_available(), reason="NEEDS THE REFERENCE TREE (build container only): "
                                                       "scripts/gen_scores_golden.py --check was NOT run")
def test_generator_check_reproduces_committed_golden():
    """what `python scripts/gen_scores_golden.py --check` does: the recipe re-run with the reference's own functions gives
    every array of the committed file, and nothing else"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "gen_scores_golden", os.path.join(os.path.dirname(__file__), "..", "scripts", "gen_scores_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = gen.generate()
    assert sorted(out) == sorted(G.files)
    assert not [k for k in out if not np.array_equal(np.asarray(out[k]), G[k])]
