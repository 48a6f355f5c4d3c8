"""the cases of tests/golden/resegmentation_ref.npz (scripts/gen_resegmentation_golden.py) and the comparison both
resegmentation test files make against them"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "resegmentation_ref.npz"))
CASES = [str(c) for c in G["cases"]]


def case_inputs(name):
    """-> (seg u8 [C, L, S], hypothesis turns, chunks, warm_up, num_samples)"""
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.der import parse_rttm
    f, key = str(G[f"{name}_src"]).split(":")
    dur, ratio, n, w = G[f"{name}_args"]
    chunks = SlidingWindow(start=0.0, duration=float(dur), step=float(ratio) * float(dur))
    return np.load(os.path.join(GOLD, f))[key], parse_rttm(G[f"{name}_hypothesis"].tobytes().decode()), chunks, float(w), int(n)


def check_against_golden(name, seg, chunks, w, count, counts, hard, discrete):
    """every artefact of one composition against the reference-made ones; `hard` through the data it moves, not its indices"""
    from diarizen_amd.postprocess import permutated_decisions, trim_frames
    from diarizen_amd.resegmentation import annotation_from_discrete
    l0, Lt = trim_frames(seg.shape[1], w)
    n = counts.shape[1]
    assert counts.dtype == np.int32 and np.array_equal(counts, G[f"{name}_counts"])
    assert np.array_equal(permutated_decisions(seg[:, l0:l0 + Lt], hard, n), G[f"{name}_permutated"])
    assert np.array_equal(np.asarray(count.data), G[f"{name}_count"])
    assert np.array_equal(np.asarray(discrete.data), G[f"{name}_discrete"])
    sw = discrete.sliding_window
    assert np.array_equal(np.array([sw.start, sw.duration, sw.step]), G[f"{name}_frames"])
    assert annotation_from_discrete(discrete, uri=name).to_rttm().encode() == G[f"{name}_rttm"].tobytes()


def boundary_ties(seg, hard, n, chunks, count):
    """bool [T]: frames where the count-th and the (count + 1)-th largest activation are equal.  There to_diarization's
    argsort (PA/pipelines/utils/diarization.py:233-238) picks by column order, in the reference too, so the chosen speaker
    depends on how the hypothesis's labels sort; on every other frame the chosen SET does not."""
    from diarizen_amd.postprocess import aggregate, permutated_decisions
    act = aggregate(permutated_decisions(seg, hard, n), chunks, count.sliding_window, missing=0.0, skip_average=True).data
    top = -np.sort(-act, axis=1)
    c = np.asarray(count.data)[:len(top), 0].astype(np.int64)
    t = np.arange(len(top))
    inside = (c > 0) & (c < n)
    return inside & (top[t, np.clip(c - 1, 0, n - 1)] == top[t, np.clip(c, 0, n - 1)])


def renamed_runs_agree(seg, turns, rename, chunks, num_samples, run):
    """the hypothesis `turns` and the same turns under `rename`d labels (another sort order: the columns move) through
    run(ref) -> (count, counts, hard, discrete): column k of one result is the column of the renamed label in the other on every
    frame without a boundary tie, and such frames are the rule.  -> the two label lists"""
    from diarizen_amd.postprocess import discretize_turns, receptive_field, reference_extent
    frames = receptive_field()
    _, Tr = reference_extent(num_samples, 16000, chunks, frames)
    out = []
    for hyp in (turns, [(a, b, rename[x]) for a, b, x in turns]):
        ref, labels = discretize_turns(hyp, frames, Tr)
        count, _, hard, discrete = run(ref)
        n = max(len(labels), seg.shape[2])
        out.append((labels, np.asarray(discrete.data), boundary_ties(seg, hard, n, chunks, count), np.asarray(count.data)))
    (l0, d0, t0, c0), (l1, d1, t1, c1) = out
    assert sorted(l1, key=str) == l1 and [rename[x] for x in l0] != l1 and sorted(rename[x] for x in l0) == l1
    col = [l1.index(rename[x]) for x in l0] + list(range(len(l0), d0.shape[1]))     # columns past K are nobody's: they stay
    assert np.array_equal(c0, c1) and d0.shape == d1.shape
    clean = ~(t0 | t1)
    assert clean.mean() > 0.8
    assert np.array_equal(d0[clean], d1[clean][:, col])
    return l0, l1
