"""Live array feeds, the host side (diarizen_amd/audio.py: Beamform(causal=True), causal_delays, beam_ready, ArrayFeedPlanner,
FeedFormat; hub.HubBook; testkit/beamform_live_ref.py: the plain-loop restatement and the signals P, Q, R): the causal delay rule
against its restatement, the conditions under which the device test (tests/test_beamform_live_gpu.py) may compare every entry
of P, Q, R without a margin, what the planner's calls tile and upload, and the refusals."""
from __future__ import annotations

import numpy as np
import pytest

from testkit import beamform_live_ref as LR
from testkit import beamform_ref as R

H = 256


# ----------------------------------------------------------------------------- the causal rule
@pytest.mark.parametrize("name", ["P", "Q", "R"])
def test_causal_delays_equal_the_reference_loop_on_the_signals(name):
    from diarizen_amd.audio import causal_delays
    c = LR.signal(name)
    lag, peak, _ = LR.reference(name)
    got = causal_delays(lag, peak, c["T"], c["hop"], c["min_peak"], LR.REFERENCE)
    assert got.dtype == np.int32 and np.array_equal(got, LR.reference_delays(name))
    assert not got[LR.REFERENCE].any() and np.abs(got).max() <= c["max_lag"]


def test_causal_delays_equal_the_reference_loop_on_random_columns():
    from diarizen_amd.audio import causal_delays
    lag, peak, T, hop, min_peak = LR.random_case()
    assert lag.shape == (4, 23) and not R.supported(T, hop)[-1]
    floor = np.float32(min_peak)
    for v in (floor, np.nextafter(floor, np.float32(0)), np.nextafter(floor, np.float32(1))):
        assert (peak[:, :-1] == v).sum() >= peak.shape[0]                         # the threshold and both neighbours occur
    for ref in (0, 2):
        want = LR.causal_delays(lag, peak, T, hop, min_peak, ref)
        assert np.array_equal(causal_delays(lag, peak, T, hop, min_peak, ref), want)
        assert not want[ref].any()
    want = LR.causal_delays(lag, peak, T, hop, min_peak, 0)
    # the last block is unsupported: its own lag, with a peak of 1, must not enter
    moved = lag.copy()
    moved[:, -1] = np.where(lag[:, -1] == 8, -8, 8)
    assert np.array_equal(causal_delays(moved, peak, T, hop, min_peak, 0), want)
    with pytest.raises(ValueError, match="causal_delays"):
        causal_delays(lag[:, :-1], peak[:, :-1], T, hop, min_peak, 0)


def _causal(lag, peak, T, min_peak=0.5, hop=H):
    from diarizen_amd.audio import causal_delays
    lag = np.array([np.zeros(len(lag), dtype=np.int64), lag])
    peak = np.array([np.zeros(len(peak)), peak], dtype=np.float32)
    out = causal_delays(lag, peak, T, hop, min_peak, 0)
    assert np.array_equal(out, LR.causal_delays(lag, peak, T, hop, min_peak, 0))
    return out[1].tolist()


def test_causal_delays_known_answers():
    from diarizen_amd.audio import smooth_delays
    # the left edge repeats the first entry: with fewer than five blocks the first held value outvotes the rest
    assert _causal([5], [1], 0) == [0]                                   # (an empty recording: its one block is unsupported)
    assert _causal([5, 1], [1, 1], 1 * H) == [5, 5]
    assert _causal([5, 1, 1], [1, 1, 1], 2 * H) == [5, 5, 5]
    assert _causal([5, 1, 1, 1], [1, 1, 1, 1], 3 * H) == [5, 5, 5, 1]
    # a change takes effect two blocks late; an isolated outlier never does
    assert _causal([2, 2, 2, 7, 7, 7, 7], [1] * 7, 6 * H) == [2, 2, 2, 2, 2, 7, 7]
    assert _causal([2, 2, 2, 9, 2, 2, 2], [1] * 7, 6 * H) == [2] * 7
    # no backward fill: the first reliable block is b = 3, the channel stays at 0 until the median turns (b = 5), where
    # smooth_delays fills the blocks before b = 3 with its lag
    lag, peak = [9, 9, 9, 4, 4, 4, 4, 4], [0, 0, 0, 1, 1, 1, 1, 1]
    assert _causal(lag, peak, 7 * H) == [0, 0, 0, 0, 0, 4, 4, 4]
    both = np.array([np.zeros(8, dtype=np.int64), lag]), np.array([np.zeros(8), peak], dtype=np.float32)
    assert smooth_delays(*both, 7 * H, H, 0.5, 0)[1].tolist() == [4] * 8
    # held across unreliable blocks; a peak equal to the threshold is reliable
    assert _causal([3, 8, 8, 8, 8, 8, 8], [0.5, 0, 0, 0, 0, 0, 0], 6 * H) == [3] * 7
    # the support rule: T = 5 H + 9 has seven blocks, the last frame holds 9 samples
    assert _causal([1, 1, 1, 1, 1, 1, 6], [1] * 7, 5 * H + 9) == [1] * 7


def test_beam_ready():
    from diarizen_amd.audio import beam_ready
    for hop in (256, 512):
        for frames in (0, 1, hop - 1, hop, 2 * hop - 1, 2 * hop, 2 * hop + 1, 7 * hop + 3):
            assert beam_ready(frames, hop) == LR.beam_ready(frames, hop)
    assert [beam_ready(r, 256) for r in (0, 255, 256, 511, 512, 768)] == [0, 0, 0, 0, 256, 512]


# ----------------------------------------------------------------------------- what lets the device test compare every entry
@pytest.mark.parametrize("name", ["P", "Q", "R"])
def test_signals_are_clear_of_the_comparison_margin(name):
    """the device transform differs from float64 by less than m = 32 E in a correlation value (tests/test_beamform_host.py
    derives E); on P, Q, R no supported entry is that close to a decision, so the device must reproduce EVERY causal delay"""
    E, m = R.comparison_margin()
    assert m == 32.0 * E and m < 1e-5
    c = LR.signal(name)
    lag, peak, margin = LR.reference(name)
    sup = R.supported(c["T"], c["hop"])
    others = np.arange(4) != LR.REFERENCE
    reliable = sup[None, :] & (peak.astype(np.float32) >= np.float32(c["min_peak"])) & others[:, None]
    assert np.abs(peak - c["min_peak"])[others][:, sup].min() > 0.05 > m             # no reliability decision can flip
    assert margin[reliable].min() > 0.03 > m                                        # no lag of a reliable entry can flip
    unreliable = sup[None, :] & ~reliable & others[:, None]
    assert unreliable.sum() >= 9 and (peak[unreliable] == 0).sum() >= 6             # held blocks, some with peak 0 exactly
    d = LR.reference_delays(name)
    assert all(len(np.unique(d[ch])) >= 2 for ch in np.flatnonzero(others))          # every channel changes delay
    l32, p32, _ = R.raw_delays(c["x"], LR.REFERENCE, c["hop"], c["max_lag"], np.float32)
    assert np.array_equal(LR.causal_delays(l32, p32, c["T"], c["hop"], c["min_peak"], LR.REFERENCE), d)
    # the signal is what an int16 feed delivers, and the silent stretches are exact zeros
    assert np.array_equal(LR.frames_of(c["x"]).T.astype(np.float32) * np.float32(2.0 ** -15), c["x"])
    assert not c["x"][1:, :2 * c["hop"] + 5].any() and c["x"][0, :2 * c["hop"] + 5].any()


# ----------------------------------------------------------------------------- the planner
def _chunkings(data: bytes, seed: int):
    g = np.random.default_rng(seed)
    yield [data]
    yield [data[i:i + 5921] for i in range(0, len(data), 5921)]
    cuts = np.sort(g.integers(0, len(data) + 1, size=12))
    parts = [data[a:z] for a, z in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(data)]]))]
    parts.insert(3, b"")                                                # empty chunks, and chunks that end inside a frame
    yield parts


def _plan_and_check(x, hop, max_lag, slot_frames, chunks, rate=16000, model_rate=16000):
    from diarizen_amd import audio
    C, T = x.shape
    fmt = audio.FeedFormat(rate, "s16", channels=C, channel=audio.Beamform(causal=True, hop=hop,
                                                                          max_delay=max_lag / rate))
    plan = audio.ArrayFeedPlanner(fmt, model_rate, slot_frames)
    assert (plan.hop, plan.max_lag) == (hop, max_lag)
    assert plan.max_upload_frames == slot_frames + 2 * hop + max_lag
    calls, fed = [], 0
    for ch in chunks:
        calls += plan.append(ch)
        fed += len(ch)
        assert plan.frames == fed // fmt.frame_bytes
        assert plan.ready == LR.beam_ready(plan.frames, hop) and plan.blocks == plan.frames // hop
    calls += plan.finish()
    assert plan.finish() == [] and plan.frames == T
    with pytest.raises(RuntimeError):
        plan.append(b"")
    raw = LR.frames_of(x).tobytes() if T else b""
    n = b = m = 0
    for c in calls:
        assert (c.n0, c.b0, c.m0) == (n, b, m) and c.n1 >= c.n0 and c.b1 > c.b0 and c.m1 >= c.m0
        n, b, m = c.n1, c.b1, c.m1
        assert c.frames <= plan.max_upload_frames and c.b1 - c.b0 <= plan.max_blocks and c.n1 - c.n0 <= plan.max_new
        assert c.first >= 0 and c.first + c.frames == c.total and len(c.data) == c.frames * fmt.frame_bytes
        assert c.data == raw[c.first * fmt.frame_bytes:c.total * fmt.frame_bytes]
        # the upload covers what the blocks read, and what the samples read with ANY delays the tracker can make
        lo, hi = audio.beamform_delays_span(c.b0, c.b1, hop, c.total)
        assert lo == hi or (c.first <= lo and hi <= c.total)
        nb_now = R.num_blocks(c.total, hop)
        for d in (-max_lag, max_lag):
            lo, hi = audio.beamform_sum_span(np.full((C, nb_now), d), hop, c.n0, c.n1, c.total)
            assert lo == hi or (c.first <= lo and hi <= c.total)
        assert c.n1 == c.n0 or (c.n1 - 1) // hop + 1 < c.b1              # every block the samples use is tracked by then
        if model_rate == rate:
            assert (c.m0, c.m1, c.s_first) == (c.n0, c.n1, c.n0)
        else:
            lo, hi = audio.resample_input_span(c.m0, c.m1, plan.o, plan.n, plan.width)
            lo, hi = max(lo, 0), min(hi, c.n1)
            assert hi <= lo or c.s_first <= lo
            assert c.s_first <= c.n0 and c.n0 - c.s_first < plan.K
    assert (n, b) == (T, R.num_blocks(T, hop))
    assert m == audio.resampled_length(T, plan.o, plan.n)
    return calls


@pytest.mark.parametrize("name", ["P", "Q", "R"])
def test_array_feed_planner_tiles_the_recording(name):
    c = LR.signal(name)
    raw = LR.frames_of(c["x"]).tobytes()
    hop = c["hop"]
    for k, slot in enumerate((1, hop - 1, hop, 3 * hop + 5)):
        for j, chunks in enumerate(_chunkings(raw, 100 * k + ord(name))):
            if slot == 1 and j == 0 and name != "P":
                continue                                                # (one frame per planned step: slow, once is enough)
            _plan_and_check(c["x"], hop, c["max_lag"], slot, chunks)
    # a trailing partial frame is carried, then dropped
    calls = _plan_and_check(c["x"], hop, c["max_lag"], hop, [raw[:1001], raw[1001:] + b"\x01\x02\x03"])
    assert calls[-1].total == c["T"]


def test_array_feed_planner_short_streams_and_two_rates():
    x = LR.signal("P")["x"]
    for T in (0, 100, H):
        raw = LR.frames_of(x[:, :T]).tobytes() if T else b""
        for chunks in ([raw], [raw[:37], raw[37:]], []):
            if T and not chunks:
                continue
            calls = _plan_and_check(x[:, :T], H, 8, H, chunks)
            assert [(c.b0, c.b1) for c in calls][-1][1] == R.num_blocks(T, H)
    r = LR.signal("R")
    raw = LR.frames_of(r["x"]).tobytes()
    for slot in (r["hop"], 3 * r["hop"] + 5):
        for chunks in _chunkings(raw, slot):
            _plan_and_check(r["x"], r["hop"], r["max_lag"], slot, chunks, rate=48000, model_rate=16000)


# ----------------------------------------------------------------------------- Beamform(causal=...), FeedFormat, the hub
def test_beamform_causal_argument():
    from diarizen_amd.audio import Beamform
    assert repr(Beamform()) == "Beamform(reference=0, max_delay=0.01, hop=None, min_peak=None)"
    assert repr(Beamform(1, 0.02, 512, 0.25)) == "Beamform(reference=1, max_delay=0.02, hop=512, min_peak=0.25)"
    assert repr(Beamform(causal=True)) == "Beamform(reference=0, max_delay=0.01, hop=None, min_peak=None, causal=True)"
    assert Beamform().causal is False and Beamform(causal=True).causal is True and Beamform(causal=np.True_).causal is True
    assert Beamform() == Beamform(causal=False) and hash(Beamform()) == hash(Beamform(causal=False))
    assert Beamform() != Beamform(causal=True) and Beamform(causal=True) == Beamform(0, 0.01, None, None, True)
    assert len({Beamform(), Beamform(causal=False), Beamform(causal=True)}) == 2
    assert Beamform(causal=True).plan(16000, 4) == Beamform().plan(16000, 4)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="Beamform: causal"):
            Beamform(causal=bad)


def test_feed_format_takes_a_causal_beamform_only():
    from diarizen_amd.audio import ArrayFeedPlanner, Beamform, FeedFormat
    bf = Beamform(causal=True, hop=256)
    fmt = FeedFormat(16000, "s16", channels=4, channel=bf)
    assert fmt.channel is bf and fmt.frame_bytes == 8 and "causal=True" in repr(fmt)
    assert FeedFormat(16000, "s16", channels=4).with_channel(bf).channel == bf       # the pipeline's channel, adopted
    assert fmt.with_channel(0).channel == bf                                         # its own choice holds
    with pytest.raises(ValueError, match="no channel code"):
        fmt.channel_code()
    for make in (lambda: FeedFormat(16000, "s16", channels=4, channel=Beamform(hop=256)),
                 lambda: FeedFormat(16000, "s16", channels=4).with_channel(Beamform())):
        with pytest.raises(ValueError, match=r"pass Beamform\(causal=True\)"):
            make()
    with pytest.raises(ValueError, match="1 channel"):
        FeedFormat(16000, "s16", channels=1, channel=bf)                              # a mono feed is no array
    with pytest.raises(ValueError, match="65 channel"):
        FeedFormat(16000, "s16", channels=65, channel=bf)
    with pytest.raises(ValueError, match="reference channel 4 of a source with 4"):
        FeedFormat(16000, "s16", channels=4, channel=Beamform(reference=4, causal=True))
    with pytest.raises(ValueError, match="ArrayFeedPlanner"):
        ArrayFeedPlanner(FeedFormat(16000, "s16", channels=4, channel=0), 16000, 256)
    with pytest.raises(ValueError, match="slot"):
        ArrayFeedPlanner(fmt, 16000, 0)


def test_hub_refuses_an_array_feed_by_name():
    from diarizen_amd.audio import Beamform, FeedFormat
    from diarizen_amd.hub import HubBook
    book = HubBook(4, 60.0, 16000, 128000, 12800, 1 << 16, 1024)
    book.new_bank = lambda rate: 0
    with pytest.raises(ValueError, match="array feed"):
        book.admit(FeedFormat(16000, "s16", channels=4, channel=Beamform(causal=True)))
    assert len(book.free) == 4                                                        # nothing was taken
    assert book.admit(FeedFormat(16000, "s16", channels=4, channel="downmix")).row == 0
