"""GCC-PHAT delay-and-sum beamforming, the host side (diarizen_amd/audio.py: Beamform, smooth_delays; testkit/beamform_ref.py:
the float64 / float32 numpy restatements): parameter validation and defaults, hand-written known answers of the delay
smoothing, properties of the restatement on the seeded cases A .. E, and the comparison margin of the device test
(tests/test_beamform_gpu.py), which is derived here from the two restatements alone."""
from __future__ import annotations

import numpy as np
import pytest

from testkit import beamform_ref as R

H = 256


def test_beamform_validation_and_defaults():
    from diarizen_amd.audio import Beamform
    for rate, hop, lag in ((8000, 2048, 80), (16000, 4096, 160), (48000, 4096, 480), (1000, 256, 10)):
        h, l, p = Beamform().plan(rate, 4)
        assert (h, l) == (hop, lag) and p == pytest.approx(8.0 / np.sqrt(2.0 * hop), rel=1e-12), rate
    assert Beamform(max_delay=1.0).plan(16000, 2)[1] == 2048                       # capped at hop / 2
    assert Beamform(max_delay=1e-6).plan(16000, 2)[1] == 1                          # at least one sample
    assert Beamform(reference=3, hop=512, min_peak=0.25).plan(16000, 4) == (512, 160, 0.25)
    assert Beamform() == Beamform(0, 0.01) and Beamform() != Beamform(1) and "reference=0" in repr(Beamform())
    for bad in (dict(reference=-1), dict(reference=True), dict(reference=1.5), dict(reference="0"), dict(max_delay=0.0),
                dict(max_delay=-1.0), dict(max_delay=float("nan")), dict(max_delay=float("inf")), dict(hop=128),
                dict(hop=8192), dict(hop=300), dict(hop=512.0), dict(hop=True), dict(min_peak=-0.1),
                dict(min_peak=float("nan"))):
        with pytest.raises(ValueError, match="Beamform"):
            Beamform(**bad)
    with pytest.raises(ValueError, match="reference channel 2 of a source with 2"):
        Beamform(reference=2).plan(16000, 2)
    with pytest.raises(ValueError, match="1 channel"):
        Beamform().plan(16000, 1)
    with pytest.raises(ValueError, match="65 channel"):
        Beamform().plan(16000, 65)


def test_check_channel_still_refuses_a_beamform():
    """live sessions and the hub settle their channel through check_channel / FeedFormat: a Beamform is a ValueError there,
    raised before anything is allocated — never a silent fall-back to channel 0"""
    from diarizen_amd.audio import Beamform, FeedFormat, check_channel
    with pytest.raises(ValueError, match="channel"):
        check_channel(Beamform())
    with pytest.raises(ValueError, match="channel"):
        FeedFormat(8000, "ulaw", channels=2).with_channel(Beamform())
    with pytest.raises(ValueError, match="channel"):
        FeedFormat(8000, "ulaw", channels=2, channel=Beamform())


def _smooth(lag, peak, T, min_peak=0.5, hop=H, ref=0):
    from diarizen_amd.audio import smooth_delays
    lag = np.array([np.zeros(len(lag), dtype=np.int64), lag])
    peak = np.array([np.zeros(len(peak)), peak], dtype=np.float32)
    out = smooth_delays(lag, peak, T, hop, min_peak, ref)
    assert out.dtype == np.int32 and out.shape == lag.shape and not out[0].any()
    return out[1].tolist()


def test_smooth_delays_known_answers():
    from diarizen_amd.audio import smooth_delays
    # hold across unreliable blocks (T = 8 H: nine blocks, all supported)
    assert _smooth([2, 2, 2, 9, 9, 9, 4, 4, 4], [1, 1, 1, 0, 0, 0, 1, 1, 1], 8 * H) == [2, 2, 2, 2, 2, 2, 4, 4, 4]
    # the threshold is inclusive and compared in float32
    assert _smooth([2, 2, 2, 9, 9, 9, 4, 4, 4], [1, 1, 1, .5, .5, .5, 1, 1, 1], 8 * H) == [2, 2, 2, 9, 9, 9, 4, 4, 4]
    assert _smooth([3] * 9, [np.float32(0.1)] * 9, 8 * H, min_peak=0.1) == [3] * 9
    # the leading fill: blocks before the first reliable one take its lag
    assert _smooth([9, 8, 5, 5, 5, 5, 5, 5, 5], [0, 0, 1, 1, 1, 1, 1, 1, 1], 8 * H) == [5] * 9
    # an isolated outlier at either end, and one inside, removed by the mirrored median of 5
    assert _smooth([8, 5, 5, 5, 5, 5, 5, 5, -7], [1] * 9, 8 * H) == [5] * 9
    assert _smooth([5, 5, 5, 5, 40, 5, 5, 5, 5], [1] * 9, 8 * H) == [5] * 9
    # (the mirror does NOT repeat the edge sample: [a, b, c, ..] is padded to [c, b | a, b, c, ..], so the first output above
    # is median(5, 5, 8, 5, 5) = 5 where a repeated edge (8, 8, 8, 5, 5) would keep the outlier); two equal samples at the edge
    # are no outlier: median(5, 8, 8, 8, 5) = 8
    assert _smooth([8, 8, 5, 5, 5, 5, 5, 5, 5], [1] * 9, 8 * H) == [8, 8, 5, 5, 5, 5, 5, 5, 5]
    # a step survives
    assert _smooth([1, 1, 1, 1, 6, 6, 6, 6, 6], [1] * 9, 8 * H) == [1, 1, 1, 1, 6, 6, 6, 6, 6]
    # the unsupported last block (T = H + 1: block 2 holds ONE sample) is never reliable, whatever its peak
    assert _smooth([5, 5, 40], [0, 0, 1], H + 1) == [0, 0, 0]
    assert _smooth([5, 7, 40], [0, 1, 1], H + 1) == [7, 7, 7]
    # T an exact multiple of H: the last block holds H samples and counts
    assert _smooth([5, 5, 40], [0, 0, 1], 2 * H) == [40, 40, 40]
    # nb < 3: no median
    assert _smooth([3, 7], [1, 1], H) == [3, 7]
    assert _smooth([3, 7], [0, 1], H) == [7, 7]
    # nothing reliable -> zeros; shorter than one hop -> nothing supported -> zeros
    assert _smooth([4] * 9, [0.4] * 9, 8 * H) == [0] * 9
    assert _smooth([4, 4], [1, 1], 100) == [0, 0]
    # the reference row is 0 whatever came in, also when it is not row 0
    out = smooth_delays(np.full((3, 9), 6), np.ones((3, 9), dtype=np.float32), 8 * H, H, 0.5, reference=2)
    assert out.tolist() == [[6] * 9, [6] * 9, [0] * 9]
    with pytest.raises(ValueError, match="smooth_delays"):
        smooth_delays(np.zeros((2, 8)), np.zeros((2, 8)), 8 * H, H, 0.5)


def test_twiddle_table():
    from diarizen_amd.audio import beamform_twiddle
    tw = beamform_twiddle(256)
    k = np.arange(256) / 512.0
    assert tw.dtype == np.float32 and tw.shape == (256, 2)
    assert np.array_equal(tw[:, 0], np.cos(2 * np.pi * k).astype(np.float32))
    assert np.array_equal(tw[:, 1], (-np.sin(2 * np.pi * k)).astype(np.float32))
    assert tw[0].tolist() == [1.0, 0.0]


def _smoothed(name):
    from diarizen_amd.audio import Beamform, smooth_delays
    c = R.case(name)
    lag, peak, _ = R.reference(name)
    min_peak = Beamform(hop=c["hop"]).plan(16000, len(c["delays"]))[2]
    return smooth_delays(lag, peak.astype(np.float32), c["x"].shape[1], c["hop"], min_peak)


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_restatement_recovers_the_delays(name):
    c = R.case(name)
    want = np.repeat(np.array(c["delays"])[:, None], R.num_blocks(c["x"].shape[1], c["hop"]), axis=1)
    assert np.array_equal(_smoothed(name), want)
    sup = R.supported(c["x"].shape[1], c["hop"])
    assert np.array_equal(R.reference(name)[0][:, sup], want[:, sup])           # raw, on every supported block


def test_restatement_short_recording_gives_zeros():
    assert not _smoothed("E").any()


def test_restatement_output_properties():
    # case C: two noiseless copies -> the aligned mean IS the source wherever both copies have it
    c = R.case("C")
    y = R.synth(c["x"], _smoothed("C"), c["hop"])
    assert y.dtype == np.float32 and np.array_equal(y[5:], c["s"][5:])
    # case A: eight copies in independent noise -> 10 log10(8) dB over one channel
    a = R.case("A")
    y = R.synth(a["x"], _smoothed("A"), a["hop"]).astype(np.float64)
    s = a["s"].astype(np.float64)
    inner = slice(160, len(s) - 160)

    def snr(z):
        return 10 * np.log10(np.sum(s[inner] ** 2) / np.sum((z[inner] - s[inner]) ** 2))
    gain = snr(y) - snr(a["x"][0].astype(np.float64))
    print(f"case A: SNR gain {gain:.3f} dB (ideal {10 * np.log10(8):.3f})")
    assert abs(gain - 10 * np.log10(8)) < 0.5


def test_comparison_margin_of_the_device_test():
    """E = the largest |peak_float32 - peak_float64| of the numpy restatements over cases A .. E, m = 32 E.  On the float64
    reference alone no supported (channel, block) entry may have its best-to-second-best margin, or its distance to the
    min_peak threshold, below m: then neither a lag nor a reliability decision of the device can hinge on rounding.
    Recorded in DESIGN.md §4.23: E = 1.99e-7, m = 6.36e-6."""
    from diarizen_amd.audio import Beamform
    E, m = R.comparison_margin()
    print(f"beamform comparison margin: E = {E:.3e}, m = {m:.3e}")
    assert 0 < E < 1e-6 and m == 32 * E
    for name in "ABCDE":
        c = R.case(name)
        _, peak, margin = R.reference(name)
        sup = R.supported(c["x"].shape[1], c["hop"])
        min_peak = Beamform(hop=c["hop"]).plan(16000, len(c["delays"]))[2]
        assert (margin[1:, sup] >= m).all(), name
        assert (np.abs(peak[1:, sup] - np.float64(np.float32(min_peak))) >= m).all(), name


def test_float32_restatement_agrees_on_lags():
    for name in "ABCDE":
        c = R.case(name)
        lag32, peak32, _ = R.raw_delays(c["x"], 0, c["hop"], c["max_lag"], np.float32)
        sup = R.supported(c["x"].shape[1], c["hop"])
        assert peak32.dtype == np.float32 and np.array_equal(lag32[:, sup], R.reference(name)[0][:, sup]), name


def test_spans():
    from diarizen_amd.audio import beamform_blocks, beamform_delays_span, beamform_sum_span
    assert [beamform_blocks(t, 256) for t in (0, 1, 256, 257, 1281)] == [1, 2, 2, 3, 7]
    assert beamform_delays_span(0, 1, 256, 1281) == (0, 256)
    assert beamform_delays_span(2, 4, 256, 1281) == (256, 1024)
    assert beamform_delays_span(6, 7, 256, 1281) == (1280, 1281)
    assert beamform_delays_span(3, 3, 256, 1281) == (0, 0)
    d = np.zeros((2, 7), dtype=np.int64)
    d[1] = [0, -8, 8, 8, 0, 0, 0]
    assert beamform_sum_span(d, 256, 0, 1, 1281) == (0, 1)                  # block 0 reads with delays 0 / 0 and 0 / -8
    assert beamform_sum_span(d, 256, 10, 20, 1281) == (2, 20)
    assert beamform_sum_span(d, 256, 256, 512, 1281) == (248, 520)
    assert beamform_sum_span(d, 256, 1280, 1281, 1281) == (1280, 1281)
    assert beamform_sum_span(d, 256, 5, 5, 1281) == (0, 0)


def test_library_exports_the_entries(built_lib):
    from diarizen_amd import _lib
    for name in ("dzn_beamform_delays", "dzn_beamform_sum", "dzn_beamform_tile"):
        assert name in _lib.EXPORTED and getattr(built_lib, name) is not None
    assert built_lib.dzn_beamform_tile() == 1024


def test_sharded_runs_are_refused(monkeypatch):
    """with more than one torch.distributed rank, open_recording(channel=Beamform()) refuses with the one-device message
    before it reads anything"""
    from diarizen_amd import dist
    from diarizen_amd.audio import Beamform
    from diarizen_amd.pipeline import open_recording
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(RuntimeError, match=r"channel=Beamform\(\.\.\.\) runs on one device.*world size 2"):
        open_recording(b"not even a file", 16000, channel=Beamform())
    with pytest.raises(RuntimeError, match="runs on one device"):
        open_recording({"audio": b"", "channel": Beamform(reference=1)}, 16000, channel=0)
