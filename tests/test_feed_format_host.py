"""Live feeds in a stored format, the host half (no device): the schedule `audio.feed_ready` against `resample_input_span`,
the planner `audio.FeedPlanner` over hard chunkings (its calls tile the output once and in order, every upload covers what
its range reads, the history stays below K frames, the uploads reassemble the input), a float64 model that evaluates every
planned call from ONLY the bytes it uploads and must equal the whole-recording model exactly, and `audio.FeedFormat`'s
refusals."""
from __future__ import annotations

import numpy as np
import pytest

from testkit.feeds import chunkings, cut_bytes, model_samples, stored_forms


def decode_choice(body: bytes, encoding: str, channels: int, channel):
    """float32 [frames]: the host decode of the channel choice (an index or "downmix") of whole stored frames"""
    from diarizen_amd.audio import _decode_frames
    return _decode_frames(body, encoding, channels, channel)


RATES = [8000, 11025, 22050, 32000, 44100, 48000, 96000]
SLOT_FRAMES = 100


@pytest.mark.parametrize("rate", RATES)
def test_schedule_against_input_span(rate):
    """for every R < 3 K + 50 and 2000 random R: the samples below ready(R) read only frames below R, sample ready(R) reads a
    frame that has not arrived, and fewer than K of the frames received are still needed"""
    from diarizen_amd.audio import feed_history, feed_ready, resample_bank, resample_input_span
    _, o, n, width = resample_bank(rate, 16000)
    K = 2 * width + o
    Rs = list(range(3 * K + 50)) + [int(r) for r in np.random.default_rng(rate).integers(0, 10 ** 9, size=2000)]
    prev = 0
    for R in Rs:
        ready = feed_ready(R, o, n, width)
        assert ready == max(0, (R - width) // o) * n and ready % n == 0
        assert resample_input_span(0, ready, o, n, width)[1] <= R
        assert resample_input_span(ready, ready + 1, o, n, width)[1] > R
        keep = feed_history(ready, o, n, width)
        assert keep == max(0, (ready // n) * o - width) == max(0, resample_input_span(ready, ready + 1, o, n, width)[0])
        assert 0 <= R - keep < K
        if R < 3 * K + 50:
            assert ready >= prev                                        # monotone
            prev = ready
    # the lag: the feed is at most width + o - 1 frames ahead of the last final sample's frame
    assert all(R - (feed_ready(R, o, n, width) // n) * o <= width + o - 1 for R in range(width, 3 * K + 50))


def test_lag_table():
    """the figures DESIGN quotes: 7 frames at 8 kHz, 21 at 48 kHz, 457 at 44.1 kHz"""
    from diarizen_amd.audio import feed_ready, resample_ratio
    lag = {}
    for rate in (8000, 48000, 44100):
        o, n, width = resample_ratio(rate, 16000)
        # frames received beyond the frame that the first sample not yet final belongs to, at its worst
        lag[rate] = max(R - (feed_ready(R, o, n, width) // n) * o for R in range(width, width + 5 * o))
        assert lag[rate] == width + o - 1
    assert lag == {8000: 7, 48000: 21, 44100: 457}


CASES = [(8000, 1500, "ulaw", 2, 1), (8000, 1500, "ulaw", 2, "downmix"), (44100, 3001, "s24", 3, 2),
         (32000, 2001, "s24", 3, "downmix"), (48000, 2400, "ulaw", 2, 0), (16000, 1203, "s24", 3, "downmix"),
         (16000, 1203, "ulaw", 2, 1)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "-".join(map(str, c)))
def case(request):
    """(format, whole body bytes with a trailing partial frame, decoded choice float32 [T], float64 model of the whole)"""
    from diarizen_amd.audio import FeedFormat, resample_bank, resampled_length
    rate, T, enc, C, ch = request.param
    fmt = FeedFormat(rate, enc, channels=C, channel=ch)
    stored, _ = stored_forms(T, C, seed=rate + T)[enc]
    body = stored.tobytes()
    assert len(body) == T * fmt.frame_bytes
    x = decode_choice(body, enc, C, ch)
    if rate == 16000:
        bank64, o, n, width, whole = None, 1, 1, 0, x.astype(np.float64)
    else:
        bank, o, n, width = resample_bank(rate, 16000)
        bank64 = bank.astype(np.float64)
        whole = model_samples(bank64, o, n, width, 0, resampled_length(T, o, n), x, 0, T)
    tail = b"\x5a" * (fmt.frame_bytes - 1)                              # a partial frame at the end: dropped
    return fmt, body + tail, T, x, (bank64, o, n, width), whole


CHUNKINGS = ["bytes", "prime", "packets", "empty", "short", "big"]


@pytest.mark.parametrize("chunking", CHUNKINGS)
def test_planner_and_numpy_model(case, chunking):
    from diarizen_amd.audio import FeedPlanner, feed_ready, resample_input_span, resampled_length
    fmt, data, T, x, (bank64, o, n, width), whole = case
    K = 2 * width + o
    plan = FeedPlanner(fmt, 16000, SLOT_FRAMES)
    assert (plan.o, plan.n, plan.width, plan.K) == (o, n, width, K) and plan.same_rate == (fmt.rate == 16000)
    fb = fmt.frame_bytes
    sizes = chunkings(len(data), fmt.rate, fb, (K - 1) * fb, SLOT_FRAMES * fb)[chunking]
    if chunking == "big":
        assert sizes[0] > (SLOT_FRAMES + K) * fb                       # larger than a slot: split
    if chunking == "short" and K > 4:
        assert max(sizes) < (K - 1) * fb
    M = resampled_length(T, o, n)
    got = np.full(M, np.nan)
    seen = bytearray(T * fb)
    covered = np.zeros(T, dtype=bool)
    at, fed = 0, 0

    def take(calls, final):
        nonlocal at
        for c in calls:
            assert c.m0 == at and c.m1 > c.m0, "ranges tile the output once and in order"
            at = c.m1
            assert len(c.data) == c.frames * fb and c.frames <= plan.max_upload_frames == SLOT_FRAMES + (K - 1 if bank64 is not None else 0)
            assert c.total <= plan.frames and c.first + c.frames == c.total      # (a split chunk: one total per piece)
            if bank64 is None:
                assert (c.first, c.frames) == (c.m0, c.m1 - c.m0)
                lo, hi = c.m0, c.m1
            else:
                assert c.m1 <= resampled_length(c.total, o, n)
                assert c.m1 == (M if final else feed_ready(c.total, o, n, width))
                lo, hi = resample_input_span(c.m0, c.m1, o, n, width)
                lo, hi = max(lo, 0), min(hi, c.total)
            assert c.first <= lo and hi <= c.first + c.frames, "the upload covers the span"
            seen[c.first * fb:(c.first + c.frames) * fb] = c.data
            covered[c.first:c.first + c.frames] = True
            xc = decode_choice(bytes(c.data), fmt.encoding, fmt.channels, fmt.channel)
            if bank64 is None:
                got[c.m0:c.m1] = xc.astype(np.float64)
            else:
                got[c.m0:c.m1] = model_samples(bank64, o, n, width, c.m0, c.m1, xc, c.first, c.total)

    for chunk in cut_bytes(data, sizes):
        take(plan.append(chunk), False)
        fed += len(chunk)
        assert plan.frames == fed // fb
        assert plan.ready == at == (plan.frames if bank64 is None else feed_ready(plan.frames, o, n, width))
        assert len(plan._hist) == (plan.frames - plan._hist_first) * fb and plan.frames - plan._hist_first < K
        assert plan.length_after(0) == resampled_length(plan.frames, o, n)
    assert plan.frames == T and len(plan._partial) == fb - 1
    take(plan.finish(), True)
    assert at == M == plan.ready and plan.finish() == []
    assert covered.all() and bytes(seen) == data[:T * fb], "the uploads reassemble the input; the partial frame is dropped"
    assert np.array_equal(got, whole), "every planned call, from its own bytes only, gives the whole-recording samples"
    with pytest.raises(RuntimeError, match="finished"):
        plan.append(b"\0")


def test_array_feeds_and_partial_frames():
    """arrays of the stored dtype are taken as their bytes; another dtype is refused; a stream shorter than one frame, or
    empty, plans nothing"""
    from diarizen_amd.audio import FeedFormat, FeedPlanner
    fmt = FeedFormat(8000, "s16", channels=2, channel=0)
    a = np.arange(-300, 300, dtype=np.int16)
    p1, p2 = FeedPlanner(fmt, 16000, 50), FeedPlanner(fmt, 16000, 50)
    c1 = p1.append(a) + p1.finish()
    c2 = p2.append(a.tobytes()) + p2.finish()
    assert [(c.first, c.frames, c.total, c.m0, c.m1, bytes(c.data)) for c in c1] == \
           [(c.first, c.frames, c.total, c.m0, c.m1, bytes(c.data)) for c in c2] and c1[-1].m1 == 600
    with pytest.raises(ValueError, match="int16"):
        p1 = FeedPlanner(fmt, 16000, 50)
        p1.append(a.astype(np.float32))
    p = FeedPlanner(fmt, 16000, 50)
    assert p.append(b"") == [] and p.append(b"\1\2\3") == [] and p.finish() == [] and (p.frames, p.ready) == (0, 0)


def test_feed_format_refusals():
    from diarizen_amd.audio import FeedFormat
    f = FeedFormat(8000, "ulaw", channels=2)
    assert (f.rate, f.encoding, f.channels, f.channel, f.frame_bytes, f.src_format) == (8000, "ulaw", 2, None, 2, 6)
    assert f.with_channel(1).channel == 1 and f.with_channel("downmix").channel_code() == -1
    assert FeedFormat(8000, "ulaw", channels=2, channel=0).with_channel(1).channel == 0      # its own choice wins
    assert FeedFormat(48000, "s24", channels=3).frame_bytes == 9
    assert FeedFormat(16000, "f32").src_format == 0 and FeedFormat(16000, "f32", channels=2).src_format == 5
    for bad in ("mp3", "s16be", "f64", None, 1):
        with pytest.raises(ValueError, match="encoding"):
            FeedFormat(8000, bad)
    for bad in (2, -1, True, "left"):
        with pytest.raises(ValueError, match="channel"):
            FeedFormat(8000, "ulaw", channels=2, channel=bad)
    with pytest.raises(ValueError, match="channel 1 of a source with 1 channel"):
        FeedFormat(8000, "ulaw").with_channel(1)                        # the pipeline's channel on a mono feed
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError):
            FeedFormat(bad, "s16")
    with pytest.raises(ValueError, match="channels"):
        FeedFormat(8000, "s16", channels=0)


def test_tile_rule_matches_the_ratios_in_use():
    """the LDS rule of the device resampler restated on the host: every rate of the schedule test fits a 1024-sample tile, a
    ratio with a huge o does not"""
    from diarizen_amd.audio import resample_bank, resample_ratio, resample_tile_fits
    for rate in RATES:
        _, o, n, width = resample_bank(rate, 16000)
        assert resample_ratio(rate, 16000) == (o, n, width) and resample_tile_fits(o, n, width, 1024)
    assert resample_ratio(15999, 16000) == (15999, 16000, 7)
    assert not resample_tile_fits(15999, 16000, 7, 1024)              # 15999 Hz -> 16 kHz: 32012 floats per tile
    assert resample_tile_fits(441, 160, 17, 1024) and not resample_tile_fits(441, 160, 17, 8192)
