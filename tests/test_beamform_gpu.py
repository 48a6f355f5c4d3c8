"""GCC-PHAT delay-and-sum beamforming on the MI355X (csrc/beamform.hip: dzn_beamform_delays, dzn_beamform_sum;
audio.BeamformedSource; pipeline.open_recording(channel=Beamform(...))).  The raw delays are compared with the float64 numpy
restatement (testkit/beamform_ref.py) inside the margin m = 32 E that tests/test_beamform_host.py derives from the two numpy
restatements; the alignment pass is compared bit for bit with the float32 restatement; range calls must equal slices of
whole-recording calls; then the library's refusals and the plumbing up to the pipelines.  At most 41 FFT blocks per case."""
from __future__ import annotations

import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from testkit import beamform_ref as R
from testkit.telephony import sphere_bytes, wav_bytes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")


def _extra_case(name):
    """beyond A .. E: D with ref = 2; three channels, T an exact multiple of the hop, max_lag = 1; max_lag = hop / 2"""
    if name == "D2":
        c = R.case("D")
        return c["x"], 2, c["hop"], c["max_lag"]
    if name == "C3":
        return R.delayed_copies(R.white(3 * 256, 0.1, 31), (0, 1, -1), 0.03, 32), 0, 256, 1
    if name == "HALF":
        return R.delayed_copies(R.white(2 * 256 + 5, 0.1, 41), (0, 100, -128), 0.03, 42), 1, 256, 128
    c = R.case(name)
    return c["x"], 0, c["hop"], c["max_lag"]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "D2", "C3", "HALF"])
def test_raw_delays_against_float64(built_lib, gpu, name):
    """on every supported (c != ref, b) entry whose float64 margin is >= m: the float64 lag, and the float64 peak within m;
    at most 1 % of the supported entries may be left out for margin; the reference row is exactly 0"""
    from diarizen_amd.audio import beamform_delays_device
    x, ref, hop, L = _extra_case(name)
    _, m = R.comparison_margin()
    lag64, peak64, margin64 = R.reference(name) if name in "ABCDE" else R.raw_delays(x, ref, hop, L, np.float64)
    lag, peak = beamform_delays_device(x, device=gpu, reference=ref, hop=hop, max_lag=L)
    nb = R.num_blocks(x.shape[1], hop)
    assert lag.shape == peak.shape == (x.shape[0], nb) and lag.dtype == torch.int32 and peak.dtype == torch.float32
    lag, peak = lag.cpu().numpy(), peak.cpu().numpy()
    assert not lag[ref].any() and not peak[ref].any()
    assert np.abs(lag).max() <= L
    use = np.repeat(R.supported(x.shape[1], hop)[None], x.shape[0], axis=0)
    use[ref] = False
    clear = use & (margin64 >= m)
    print(f"{name}: {use.sum()} supported entries, {clear.sum()} with margin >= m = {m:.2e}, "
          f"max |peak - peak64| = {np.abs(peak - peak64)[clear].max(initial=0):.2e}")
    assert use.sum() - clear.sum() <= 0.01 * use.sum()
    assert np.array_equal(lag[clear], lag64[clear])
    assert (np.abs(peak.astype(np.float64) - peak64)[clear] <= m).all()


def test_silence_and_identical_channels(built_lib, gpu):
    from diarizen_amd.audio import beamform_delays_device
    _, m = R.comparison_margin()
    kw = dict(device=gpu, reference=0, hop=256, max_lag=8)
    lag, peak = beamform_delays_device(np.zeros((4, 3 * 256 + 9), dtype=np.float32), **kw)
    assert lag.shape == (4, 5) and not lag.any() and torch.equal(peak, torch.zeros_like(peak))
    x = np.array(R.case("D")["x"])
    want = beamform_delays_device(x, **kw)
    x[1] = 0
    lag, peak = beamform_delays_device(x, **kw)
    assert not lag[1].any() and torch.equal(peak[1], torch.zeros_like(peak[1]))
    for c in (2, 3):                                    # the other channels do not notice
        assert torch.equal(lag[c], want[0][c]) and torch.equal(peak[c], want[1][c])
    same = np.repeat(R.white(5 * 256 + 1, 0.1, 5)[None], 3, axis=0)
    lag, peak = beamform_delays_device(same, **kw)
    sup = torch.from_numpy(R.supported(same.shape[1], 256)).to(gpu)      # (the last frame holds one sample, under a zero of the window)
    assert not lag.any() and (peak[1:] <= 1 + m).all() and (peak[1:, sup] > 0.99).all()


def test_delay_ranges_equal_slices(built_lib, gpu):
    """case B: blocks [0, 1), [1, 5), [b, nb), the last block alone and [0, nb), each given only the frames it reads"""
    from diarizen_amd.audio import beamform_delays_device, beamform_delays_span
    c = R.case("B")
    x, hop, L = c["x"], c["hop"], c["max_lag"]
    T = x.shape[1]
    nb = R.num_blocks(T, hop)
    whole = beamform_delays_device(x, device=gpu, reference=0, hop=hop, max_lag=L)
    for b0, b1 in ((0, 1), (1, 5), (17, nb), (nb - 1, nb), (0, nb)):
        lo, hi = beamform_delays_span(b0, b1, hop, T)
        assert (lo > 0 or b0 <= 1) and (hi < T or b1 >= nb - 1)
        part = beamform_delays_device(x[:, lo:hi], device=gpu, reference=0, hop=hop, max_lag=L, total=T, first_index=lo,
                                      blocks=(b0, b1))
        assert part[0].shape == (4, b1 - b0)
        assert torch.equal(part[0], whole[0][:, b0:b1]) and torch.equal(part[1], whole[1][:, b0:b1]), (b0, b1)


@pytest.mark.parametrize("shape", ["A", "D", "E"])
@pytest.mark.parametrize("channels", [2, 3, 8])
def test_alignment_pass_bit_for_bit(built_lib, gpu, shape, channels):
    """dzn_beamform_sum == the float32 restatement (torch.equal) with random integer delays in [-L, L] that change at every
    block and include +-L; ranges one sample either side of block edges and of the kernel's tile edges, [0, 1), [T - 1, T)
    and the whole recording, each given only the span it reads, equal slices of the whole call"""
    from diarizen_amd.audio import beamform_sum_device, beamform_sum_span, beamform_tile
    c = R.case(shape)
    T, hop, L = c["x"].shape[1], c["hop"], c["max_lag"]
    g = np.random.default_rng(100 * channels + ord(shape))
    x = (0.1 * g.standard_normal((channels, T))).astype(np.float32)
    nb = R.num_blocks(T, hop)
    delays = g.integers(-L, L + 1, size=(channels, nb)).astype(np.int32)
    delays[0] = 0
    delays[1, 0], delays[1, -1], delays[-1, 0] = L, -L, -L
    want = torch.from_numpy(R.synth(x, delays, hop))
    whole = beamform_sum_device(x, delays, device=gpu, hop=hop)
    assert whole.shape == (T,) and torch.equal(whole.cpu(), want)
    assert torch.equal(beamform_sum_device(torch.from_numpy(x).to(gpu), torch.from_numpy(delays).to(gpu), device=gpu, hop=hop),
                       whole)
    tile = beamform_tile()
    ranges = {(0, 1), (T - 1, T), (0, T)}
    for e in (hop, 2 * hop, tile, 2 * tile, 3 + tile):
        ranges |= {(e - 1, e + 1), (e, min(T, e + hop)), (max(0, e - tile), e), (3, e + 1)}
    ranges = sorted((a, z) for a, z in ranges if 0 <= a < z <= T)
    assert len(ranges) >= 3
    for n0, n1 in ranges:
        lo, hi = beamform_sum_span(delays, hop, n0, n1, T)
        part = beamform_sum_device(x[:, lo:hi], delays, device=gpu, hop=hop, total=T, first_index=lo, out_range=(n0, n1))
        assert part.shape == (n1 - n0,) and torch.equal(part, whole[n0:n1]), (n0, n1)


def test_refusals(built_lib, gpu):
    """every parameter refusal of dzn_beamform_delays / dzn_beamform_sum raises DznError with the library's message, and the
    output buffers, filled before the call, are untouched"""
    from diarizen_amd import _lib
    from diarizen_amd._lib import DznError
    from diarizen_amd.audio import _device_twiddle
    T, hop, L, ch = 5 * 256 + 1, 256, 8, 4
    nb = R.num_blocks(T, hop)
    x = torch.from_numpy(np.array(R.case("D")["x"])).to(gpu)
    x65 = torch.zeros((65, 16), device=gpu)
    lag = torch.full((65, nb), 77, device=gpu, dtype=torch.int32)
    peak = torch.full((65, nb), 7.0, device=gpu)
    dst = torch.full((T,), 7.0, device=gpu)
    good = torch.zeros((ch, nb), device=gpu, dtype=torch.int32)
    far = good.clone()
    far[2, 3] = hop // 2 + 1
    tw = _device_twiddle(hop, gpu)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def delays(x=x, channels=ch, stride=T, first=0, length=T, total=T, ref=0, hop=hop, max_lag=L, b0=0, b1=nb):
        _lib.check(built_lib.dzn_beamform_delays(gpu.index, p(x), channels, stride, first, length, total, ref, hop, max_lag,
                                                 p(tw), b0, b1, p(lag), p(peak), st), None, "dzn_beamform_delays")

    def summed(x=x, channels=ch, stride=T, first=0, length=T, total=T, hop=hop, d=good, blocks=nb, n0=0, n1=T):
        _lib.check(built_lib.dzn_beamform_sum(gpu.index, p(x), channels, stride, first, length, total, hop, p(d), blocks, n0, n1,
                                              p(dst), st), None, "dzn_beamform_sum")

    for call in (delays, summed):
        with pytest.raises(DznError, match="1 channel"):
            call(channels=1)
        with pytest.raises(DznError, match="65 channel"):
            call(x=x65, channels=65, stride=16, length=16, total=16)
        for bad in (128, 300, 8192, 0):
            with pytest.raises(DznError, match=f"hop {bad} is not a power of two"):
                call(hop=bad)
        with pytest.raises(DznError, match="ch_stride"):
            call(stride=T - 1)
    for bad in (-1, ch):
        with pytest.raises(DznError, match=f"reference channel {bad} of a source with 4"):
            delays(ref=bad)
    for bad in (0, hop // 2 + 1):
        with pytest.raises(DznError, match=f"max_lag {bad} is outside"):
            delays(max_lag=bad)
    for b0, b1 in ((0, nb + 1), (-1, 2), (3, 2)):
        with pytest.raises(DznError, match="blocks .* are not inside the 7 blocks"):
            delays(b0=b0, b1=b1)
    for n0, n1 in ((0, T + 1), (-1, 2), (3, 2)):
        with pytest.raises(DznError, match="samples .* are not inside the recording"):
            summed(n0=n0, n1=n1)
    with pytest.raises(DznError, match="num_blocks = 6, a recording of 1281 samples has 7"):
        summed(blocks=nb - 1)
    with pytest.raises(DznError, match="delay 129 of channel 2 in block 3 is beyond hop / 2 = 128"):
        summed(d=far)
    with pytest.raises(DznError, match=r"the span given, \[256, 1281\), does not cover the input \[0, 512\)"):
        delays(first=256, length=T - 256, b0=0, b1=2)
    with pytest.raises(DznError, match=r"the span given, \[0, 511\), does not cover the input \[256, 1024\)"):
        delays(length=511, b0=2, b1=4)
    with pytest.raises(DznError, match=r"the span given, \[0, 511\), does not cover the input \[500, 512\)"):
        summed(length=511, n0=500, n1=512)
    shifted = good.clone()
    shifted[1, 1] = -8
    with pytest.raises(DznError, match=r"the span given, \[256, 1281\), does not cover the input \[248, 300\)"):
        summed(first=256, length=T - 256, d=shifted, n0=256, n1=300)
    torch.cuda.synchronize()
    assert (lag == 77).all() and (peak == 7.0).all() and (dst == 7.0).all()
    summed(d=shifted)                                    # a valid call still goes through, and a block before the delay is fine
    delays()
    torch.cuda.synchronize()
    assert not (dst == 7.0).all() and not (lag[:ch] == 77).any()


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def array(tmp_path_factory):
    """case C over the full 30 s fixture — channel 1 = channel 0 advanced by 5 samples, no noise — as a two-channel int16 WAV
    and SPHERE file at 16 kHz and the same frames labelled 8 kHz; -> (wav, sph, wav8k, float32 [2, T])"""
    s = R.golden_wav()
    x = R.delayed_copies(s, (0, -5), 0.0, 0)
    pcm = np.ascontiguousarray((x.T * 32768.0).astype("<i2"))
    assert np.array_equal(pcm.T.astype(np.float32) / 32768.0, x)
    d = tmp_path_factory.mktemp("array")
    (d / "array.wav").write_bytes(wav_bytes(1, 2, 16000, 16, pcm.tobytes()))
    (d / "array.sph").write_bytes(sphere_bytes("pcm", 2, 16000, 2, pcm.tobytes()))
    (d / "array8k.wav").write_bytes(wav_bytes(1, 2, 8000, 16, pcm.tobytes()))
    return str(d / "array.wav"), str(d / "array.sph"), str(d / "array8k.wav"), x


@pytest.fixture(scope="module")
def restated(array):
    """the float32 restatement of the beamformed recording: delays [0, -5] on every block"""
    x = array[3]
    delays = np.repeat(np.array([[0], [-5]], dtype=np.int32), R.num_blocks(x.shape[1], 4096), axis=1)
    return delays, R.synth(x, delays, 4096)


@pytest.fixture(scope="module")
def pipe(gpu):
    """seeded weights as in tests/test_telephony_gpu.py; built with channel=Beamform()"""
    from diarizen_amd.audio import Beamform
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    p = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                         seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0), channel=Beamform())
    yield p
    p.close()


def test_open_recording_beamformed(built_lib, gpu, array, restated):
    from diarizen_amd.audio import Beamform, BeamformedSource
    from diarizen_amd.pipeline import open_recording
    wav, sph, _, x = array
    delays, want = restated
    T = x.shape[1]
    for path in (wav, sph, {"audio": wav, "channel": Beamform()}):
        src = open_recording(path, 16000, device=gpu, channel=0 if isinstance(path, dict) else Beamform())
        assert isinstance(src, BeamformedSource) and src.sample_rate == 16000 and src.num_samples == T
        assert src.delays is None
        whole = src.read_device(0, T)
        assert np.array_equal(src.delays, delays) and src.lags.shape == src.peaks.shape == delays.shape
        assert whole.shape == (T,) and torch.equal(whole.cpu(), torch.from_numpy(want))
        half = T // 2 + 3
        assert torch.equal(src.read_device(0, half), whole[:half]) and torch.equal(src.read_device(half, T), whole[half:])
    # a span shorter than the recording walks the same samples: the bits do not depend on the span
    src = open_recording(wav, 16000, device=gpu, channel=Beamform())
    src.SPAN = 1 << 16
    assert torch.equal(src.read_device(0, T), whole) and np.array_equal(src.delays, delays)
    # bytes in memory go through the whole-file decoder
    with open(wav, "rb") as f:
        src = open_recording(f.read(), 16000, device=gpu, channel=Beamform())
    assert isinstance(src, BeamformedSource) and torch.equal(src.read_device(0, T), whole)
    with pytest.raises(ValueError, match="reference channel 2 of a source with 2"):
        open_recording(wav, 16000, device=gpu, channel=Beamform(reference=2))
    with pytest.raises(ValueError, match="1 channel"):
        open_recording(WAV, 16000, device=gpu, channel=Beamform())


def test_device_stage_and_pipelines(built_lib, gpu, array, restated, pipe):
    from diarizen_amd.audio import Beamform, FeedFormat
    from diarizen_amd.core import Annotation
    from diarizen_amd.detection import VoiceActivityDetection
    from diarizen_amd.pipeline import open_recording
    wav, sph, wav8k, x = array
    _, want = restated
    seg0, emb0 = pipe.device_stage(want)
    assert seg0.any()
    for path in (wav, sph):
        seg, emb = pipe.device_stage(open_recording(path, 16000, device=gpu, channel=Beamform()))
        assert seg.shape == seg0.shape and np.array_equal(seg, seg0) and np.array_equal(emb, emb0), path
    assert pipe.channel == Beamform()
    ann = pipe(wav, sess_name="array")
    assert isinstance(ann, Annotation) and len(ann.labels()) >= 1
    try:
        pipe.channel = 0
        assert pipe({"audio": wav, "channel": Beamform()}, sess_name="array").to_rttm() == ann.to_rttm()
    finally:
        pipe.channel = Beamform()
    vad = VoiceActivityDetection(pipe)
    assert vad.channel == Beamform()
    speech = vad(sph)
    assert isinstance(speech, Annotation) and speech.labels() == ["SPEECH"]
    assert VoiceActivityDetection(pipe, channel=Beamform(reference=1)).channel == Beamform(reference=1)
    # the same frames at 8 kHz: beamformed at 8 kHz (hop 2048), then resampled on the device
    src = open_recording(wav8k, 16000, device=gpu, channel=Beamform())
    assert (src.hop, src.max_lag) == (2048, 80) and src.num_samples == 2 * x.shape[1]
    whole = src.read_device(0, src.num_samples)
    assert whole.shape == (2 * x.shape[1],) and torch.isfinite(whole).all() and whole.abs().max() > 0.01
    assert torch.equal(src.read_device(12345, 100000), whole[12345:112345])
    assert (src.delays[1] == -5).all()
    seg, _ = pipe.device_stage(src)
    assert seg.any()
    # live sessions keep refusing it, before anything is allocated
    before = torch.cuda.memory_allocated(gpu)
    with pytest.raises(ValueError, match="channel"):
        pipe.open_live(feed_format=FeedFormat(8000, "ulaw", channels=2))
    assert torch.cuda.memory_allocated(gpu) == before
