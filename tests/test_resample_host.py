"""Host side of the device resampler (CPU): the filter bank that `audio.resample` and csrc/resample.hip share, the index
arithmetic of a range call, and the length a ResampledSource reports."""
from __future__ import annotations

import math

import numpy as np
import pytest

from testkit.resample_ref import CASES, assert_within_bound, case_input, reference


@pytest.mark.parametrize("rate,o,n,width,K", [(48000, 3, 1, 19, 41), (44100, 441, 160, 17, 475), (22050, 441, 320, 9, 459),
                                              (32000, 2, 1, 13, 28), (8000, 1, 2, 7, 15)])
def test_bank_geometry(rate, o, n, width, K):
    from diarizen_amd.audio import resample_bank
    bank, o_, n_, width_ = resample_bank(rate, 16000)
    assert (o_, n_, width_) == (o, n, width)
    assert bank.shape == (n, K) and bank.dtype == np.float32 and K == 2 * width + o
    # torchaudio's `_get_sinc_resample_kernel`, written out independently in float64 and cast (the bank `resample` applies)
    base = min(o, n) * 0.99
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    t = np.clip((np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx) * base, -6, 6)
    window = np.cos(t * math.pi / 6 / 2) ** 2
    tp = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tp == 0, 1.0, np.sin(tp) / tp)
    want = (sinc * window * (base / o)).astype(np.float32)
    assert np.abs(bank.astype(np.float64) - want).max() <= 2.0 ** -24       # numpy's and torch's sin / cos: one rounding apart
    

@pytest.mark.parametrize("rate,T", CASES)
def test_host_resample_within_the_dot_product_bound(rate, T):
    """`resample`, now built on resample_bank, against the float64 sum over the same bank: inside the bound that the device
    kernel is held to (tests/test_resample_gpu.py), every output sample, and of length ceil(n T / o)"""
    from diarizen_amd.audio import resample, resample_bank, resampled_length
    bank, o, n, width = resample_bank(rate, 16000)
    x = case_input(rate, T)
    y = resample(x, rate, 16000)
    assert len(y) == math.ceil(n * T / o) == resampled_length(T, o, n)
    ref, mag = reference(x, bank, o, n, width)
    assert_within_bound(y, ref, mag, bank.shape[1], f"host {rate} T={T}")


def _brute_span(m0, m1, o, n, width):
    K = 2 * width + o
    read = [(m // n) * o + j - width for m in range(m0, m1) for j in range(K)]
    return min(read), max(read) + 1


@pytest.mark.parametrize("rate,T", [(48000, 4800), (44100, 22050), (22050, 5000), (8000, 777), (32000, 3001)])
def test_input_span_equals_enumeration(rate, T):
    from diarizen_amd.audio import resample_bank, resample_input_span, resampled_length
    _, o, n, width = resample_bank(rate, 16000)
    M = resampled_length(T, o, n)
    ranges = [(0, 1), (0, 7), (0, M), (M - 1, M), (M - 5, M), (M // 2, M // 2 + 1), (M // 3, M // 3 + 2 * n + 1),
              (n, 2 * n), (n - 1, n + 1)]
    for m0, m1 in ranges:
        assert 0 <= m0 < m1 <= M
        assert resample_input_span(m0, m1, o, n, width) == _brute_span(m0, m1, o, n, width), (m0, m1)
    lo, hi = resample_input_span(0, M, o, n, width)
    assert lo == -width and hi >= T            # the whole output reads below 0 and up to (or beyond) the end
    assert resample_input_span(5, 5, o, n, width) == (0, 0)


@pytest.mark.parametrize("rate,T", CASES)
def test_resampled_source_length(rate, T):
    from diarizen_amd.audio import ResampledSource, resample
    x = case_input(rate, T)
    src = ResampledSource(x, 16000, "cuda:0", orig_rate=rate)
    assert src.sample_rate == 16000
    assert src.num_samples == len(resample(x, rate, 16000))


def test_resampled_source_of_a_wav_file(tmp_path):
    """num_samples of a wrapped WavSource, and read_raw: the interleaved int16 frames as stored; None for other formats"""
    import struct
    from diarizen_amd.audio import ResampledSource, WavSource, load_wav, resample
    pcm = (np.random.default_rng(3).integers(-30000, 30000, size=(4801, 2))).astype("<i2")

    def wav(path, tag, bits, body):
        nch, sr = 2, 48000
        fmt = struct.pack("<HHIIHH", tag, nch, sr, sr * nch * bits // 8, nch * bits // 8, bits)
        path.write_bytes(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt +
                         b"data" + struct.pack("<I", len(body)) + body)
        return path
    p = wav(tmp_path / "s16.wav", 1, 16, pcm.tobytes())
    src = WavSource(p, channel=1)
    assert np.array_equal(src.read_raw(0, 10 ** 9), pcm)
    assert np.array_equal(src.read_raw(100, 7), pcm[100:107])
    assert np.array_equal(src.read_raw(4800, 5), pcm[4800:])
    assert src.read_raw(5000, 5).shape == (0, 2)
    assert np.array_equal(src.read_raw(0, 4801)[:, 1].astype(np.float32) * np.float32(2.0 ** -15), load_wav(str(p))[0][1])
    rs = ResampledSource(src, 16000, "cuda:0")
    assert rs.num_samples == len(resample(load_wav(str(p))[0][1], 48000, 16000)) == 1601
    f32 = wav(tmp_path / "f32.wav", 3, 32, (pcm / 32768.0).astype("<f4").tobytes())
    assert WavSource(f32).read_raw(0, 10) is None
    with pytest.raises(ValueError):
        ResampledSource(WavSource(p), 48000, "cuda:0")


def test_open_recording_keeps_the_host_default(tmp_path):
    """resample="host" is the default and `open_recording` refuses anything but the two names"""
    import inspect
    from diarizen_amd.pipeline import DiariZenPipeline, open_recording
    assert inspect.signature(open_recording).parameters["resample"].default == "host"
    assert inspect.signature(DiariZenPipeline.__init__).parameters["resample"].default == "host"
    with pytest.raises(ValueError):
        open_recording(b"", 16000, resample="gpu")
