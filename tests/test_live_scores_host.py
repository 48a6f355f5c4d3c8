"""Live per-speaker activity scores, the part that needs no device: postprocess.speaker_scores_range — the restatement of
dzn_diarize_range_scores' scores for a fixed number of columns and a frame range — against the reference-made
tests/golden/scores_ref.npz bit for bit over partitions of [0, T); extra columns are zeros and change nothing; StreamRows with
a float32 row; the `scores=` keyword is validated before anything is allocated; the C entry is exported and declared."""
import os

import numpy as np
import pytest

from _live_scores_cases import AGG, bits, bounds, case, partitions


def ranged(d, cuts, K=None, T=None, hard=None):
    from diarizen_amd.postprocess import speaker_scores_range
    K, T = d["K"] if K is None else K, d["T"] if T is None else T
    parts = [speaker_scores_range(d["soft"], d["hard"] if hard is None else hard, d["starts"], a, b, K, d["duration"],
                                  warm_up=d["warm_up"]) for a, b in bounds(T, cuts)]
    for (a, b), p in zip(bounds(T, cuts), parts):
        assert p.dtype == np.float32 and p.shape == (b - a, K)
    return np.concatenate(parts)


@pytest.mark.parametrize("name", AGG)
def test_range_calls_over_a_partition_equal_the_reference_run(name):
    d = case(name)
    parts = partitions(d)
    assert len(parts["window_edges"]) >= (1 if len(d["starts"]) > 1 or d["T"] > d["soft"].shape[1] else 0)
    for what, cuts in parts.items():
        got = ranged(d, cuts)
        assert np.array_equal(bits(got), bits(d["ref"])), (name, what)


@pytest.mark.parametrize("name", AGG)
def test_whole_range_equals_speaker_scores_on_every_frame(name):
    from diarizen_amd.postprocess import receptive_field, speaker_scores
    d = case(name)
    host = speaker_scores(d["soft"], d["chunks"], receptive_field(), d["hard"], warm_up=d["warm_up"]).data
    assert len(host) == d["full"] >= d["T"]
    assert np.array_equal(bits(ranged(d, [], T=d["full"])), bits(host))
    # beyond the last covered frame: no window, zeros
    tail = ranged(d, [d["full"]], T=d["full"] + 3)[d["full"]:]
    assert tail.shape == (3, d["K"]) and not tail.any()


@pytest.mark.parametrize("name", ["w2s_c12_s4_k5", "w2s_c7_padded", "w2s_c12_warm_up"])
def test_more_columns_are_zeros_and_change_no_other_bit(name):
    d = case(name)
    K = d["K"]
    wide = ranged(d, partitions(d)["window_edges"], K=K + 3)
    assert np.array_equal(bits(wide[:, :K]), bits(d["ref"])) and not wide[:, K:].any()
    assert np.array_equal(bits(ranged(d, [], K=20 if K <= 20 else 32)[:, :K]), bits(d["ref"]))
    # fewer columns: labels >= K match no column, the columns that stay keep their bits
    if K > 1:
        assert np.array_equal(bits(ranged(d, [], K=K - 1)), bits(d["ref"][:, :K - 1]))
    # no label at all: every column zero
    assert not ranged(d, [], hard=np.full_like(d["hard"], -2)).any()


def test_a_nan_is_a_missing_entry():
    """np.max propagates the NaN: that window's entry for the column is missing, as when the window has no such speaker"""
    from diarizen_amd.postprocess import speaker_scores_range
    d = case("w2s_c12_s4_k5")
    c = 3
    k = int(d["hard"][c][d["hard"][c] >= 0][0])
    soft = d["soft"].copy()
    s = int(np.nonzero(d["hard"][c] == k)[0][0])
    soft[c, 10, s] = np.nan
    t = int(d["starts"][c]) + 10
    got = speaker_scores_range(soft, d["hard"], d["starts"], 0, d["T"], d["K"], d["duration"])
    hard = d["hard"].copy()
    assert np.isfinite(got).all()
    other = np.ones(got.shape, bool)
    other[t, k] = False
    assert np.array_equal(bits(got)[other], bits(d["ref"])[other]) and got[t, k] != d["ref"][t, k]
    # window c without that speaker in that frame: drop the label from window c for a one-frame range
    hard[c][hard[c] == k] = -2
    want = speaker_scores_range(d["soft"], hard, d["starts"], t, t + 1, d["K"], d["duration"])
    assert bits(want)[0, k] == bits(got)[t, k]


def test_stream_rows_with_a_float32_row_grow_and_commit():
    from diarizen_amd.streaming import StreamRows
    K = 20
    rows = StreamRows(act=(np.uint8, (K,)), cnt=(np.uint8, ()), score=(np.float32, (K,)))
    g = np.random.default_rng(3)
    full = g.random((3000, K), dtype=np.float32)
    t0, t1, f = rows.span(700, 400)
    assert (t0, t1, f) == (0, 700, 400)
    rows.write(t0, t1, f, act=np.ones((700, K), np.uint8), cnt=np.ones(700, np.uint8), score=full[:700])
    first = rows.committed("score")
    assert first.dtype == np.float32 and first.shape == (400, K) and rows.valid("score").shape == (700, K)
    t0, t1, f = rows.span(3000, 2600)                               # past the first 1024 rows: the arrays double
    assert (t0, t1, f) == (400, 3000, 2600)
    rows.write(t0, t1, f, act=np.ones((2600, K), np.uint8), cnt=np.ones(2600, np.uint8), score=full[400:3000])
    got = rows.committed("score")
    assert got.shape == (2600, K) == rows.committed("act").shape and np.array_equal(bits(got), bits(full[:2600]))
    assert np.array_equal(bits(got[:400]), bits(first))             # committed rows only grow
    got[:] = -1.0                                                   # a copy
    assert np.array_equal(bits(rows.valid("score")), bits(full))
    t0, t1, f = rows.span(3000, 3000)                               # finish: nothing new to compute, everything committed
    rows.write(t0, t1, f)
    assert rows.committed("score").shape == (3000, K)


def test_scores_keyword_is_validated_before_anything_is_allocated():
    from diarizen_amd.live import LiveDiarization, check_scores, place_columns
    assert check_scores(True) is True and check_scores(False) is False and check_scores(np.bool_(True)) is True
    for bad in (1, 0, "yes", None, 0.5, [True]):
        with pytest.raises(ValueError, match="scores is True or False"):
            check_scores(bad)
    with pytest.raises(ValueError, match="scores is True or False"):
        LiveDiarization(None, "x", scores="yes")                    # refused before the pipeline is touched
    data = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = place_columns(data, {0: 2, 1: 0, 2: 21}, 20)
    assert out.shape == (4, 22) and out.dtype == np.float32
    assert np.array_equal(out[:, 2], data[:, 0]) and np.array_equal(out[:, 0], data[:, 1]) and np.array_equal(out[:, 21], data[:, 2])
    assert not out[:, [1] + list(range(3, 21))].any()
    assert place_columns(data[:, :1], {0: 4}, 20).shape == (4, 20)


def test_streaming_session_validates_return_scores():
    from diarizen_amd.streaming import StreamingSession
    with pytest.raises(ValueError, match="return_scores is True or False"):
        StreamingSession(None, "x", return_scores=1)


def test_symbol_is_exported_and_declared(built_lib):
    from diarizen_amd import _lib
    assert "dzn_diarize_range_scores" in _lib.EXPORTED and hasattr(built_lib, "dzn_diarize_range_scores")
    assert len(built_lib.dzn_diarize_range_scores.argtypes) == 18
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dzn.h")).read()
    assert "int dzn_diarize_range_scores(const uint8_t* d_seg, const int8_t* d_hard, const float* d_soft," in header
