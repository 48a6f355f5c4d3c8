"""The device resampler (csrc/resample.hip, dzn_resample, audio.resample_device / ResampledSource) on the MI355X: accuracy
of every output sample against the float64 sum, bit identity of a range call with a slice of the whole-recording call, the
int16 input form, the library's refusals, and the plumbing up to the pipeline (seeded weights of testkit/)."""
from __future__ import annotations

import copy
import math
import os
import struct

import numpy as np
import pytest
import torch

from testkit.resample_ref import CASES, assert_within_bound, case_input, reference

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")


@pytest.mark.parametrize("rate,T", CASES)
def test_every_sample_within_the_dot_product_bound(built_lib, gpu, rate, T):
    """|y[m] - ref[m]| <= K 2^-24 sum_j |k32[p, j]| |x32[..]|, the bound of an fp32 dot product of K terms in any order
    (exactly 0 where the sum is 0), on all ceil(n T / o) samples.  The host resampler's worst error is 0.26 of it
    (tests/test_resample_host.py prints it)."""
    from diarizen_amd.audio import resample_bank, resample_device
    bank, o, n, width = resample_bank(rate, 16000)
    x = case_input(rate, T)
    y = resample_device(x, rate, 16000, device=gpu)
    assert y.dtype == torch.float32 and y.device.type == "cuda"
    assert y.shape == (math.ceil(n * T / o),)
    ref, mag = reference(x, bank, o, n, width)
    assert_within_bound(y.cpu().numpy(), ref, mag, bank.shape[1], f"device {rate} T={T}")
    # a device tensor as input gives the same bits as the host array
    assert torch.equal(resample_device(torch.from_numpy(x).to(gpu), rate, 16000, device=gpu), y)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_range_call_equals_slice_of_the_whole_call(built_lib, gpu, rate):
    """resample_device(out_range=(m0, m1)) given ONLY resample_input_span of the input == whole[m0:m1], bit for bit: ranges
    from 0, to the last sample, one sample either side of tile edges (relative to the range and to the whole call), and of
    one sample; the recording spans three tiles and a ragged tail"""
    from diarizen_amd.audio import resample_bank, resample_device, resample_input_span, resample_tile
    tile = resample_tile()
    assert tile > 0
    _, o, n, width = resample_bank(rate, 16000)
    M = 3 * tile + 137
    T = (M * o) // n - 1                                   # ceil(n T / o) == M, T no multiple of o
    assert math.ceil(n * T / o) == M
    x = (0.3 * np.random.default_rng(rate).standard_normal(T)).astype(np.float32)
    whole = resample_device(x, rate, 16000, device=gpu)
    assert whole.shape == (M,)
    ranges = [(0, M), (0, 1), (0, tile), (0, tile - 1), (0, tile + 1), (tile - 1, 2 * tile + 1), (tile + 1, 2 * tile - 1),
              (tile, 3 * tile), (1, tile + 1), (2 * tile - 1, 2 * tile), (2 * tile, 2 * tile + 1), (3 * tile - 1, M),
              (3 * tile + 1, M), (M - 1, M), (tile // 2 + 3, tile // 2 + 4), (7, M - 7)]
    for m0, m1 in ranges:
        lo, hi = resample_input_span(m0, m1, o, n, width)
        lo, hi = max(lo, 0), min(hi, T)
        part = resample_device(x[lo:hi], rate, 16000, device=gpu, out_range=(m0, m1), total=T, first_index=lo)
        assert part.shape == (m1 - m0,)
        assert torch.equal(part, whole[m0:m1]), (m0, m1)


@pytest.mark.parametrize("rate,T", [(48000, 4800), (44100, 3001), (32000, 3001)])
def test_int16_stereo_equals_the_float_path(built_lib, gpu, rate, T):
    """interleaved int16 frames, channel 0 and channel 1 selected by the kernel == the float32 path on x / 32768"""
    from diarizen_amd.audio import resample_device
    pcm = np.random.default_rng(T).integers(-32768, 32768, size=(T, 2)).astype(np.int16)
    for ch in (0, 1):
        want = resample_device((pcm[:, ch] / 32768.0).astype(np.float32), rate, 16000, device=gpu)
        got = resample_device(pcm, rate, 16000, device=gpu, channels=2, channel=ch)
        assert torch.equal(got, want), ch
        assert torch.equal(resample_device(torch.from_numpy(pcm.reshape(-1)).to(gpu), rate, 16000, device=gpu, channels=2,
                                           channel=ch), want)


def test_refusals(built_lib, gpu):
    """a span that is too short, channel == channels and m1 beyond the output length raise with the library's message, and
    nothing is launched: the output of an earlier call and the device stay untouched"""
    from diarizen_amd._lib import DznError
    from diarizen_amd.audio import resample_bank, resample_device, resample_input_span
    _, o, n, width = resample_bank(48000, 16000)
    T = 4800
    x = case_input(48000, T)
    lo, hi = resample_input_span(500, 600, o, n, width)
    with pytest.raises(DznError, match="does not cover"):
        resample_device(x[lo + 1:hi], 48000, 16000, device=gpu, out_range=(500, 600), total=T, first_index=lo + 1)
    with pytest.raises(DznError, match="does not cover"):
        resample_device(x[lo:hi - 1], 48000, 16000, device=gpu, out_range=(500, 600), total=T, first_index=lo)
    pcm = np.zeros((T, 2), dtype=np.int16)
    with pytest.raises(DznError, match="channel 2 of a source with 2"):
        resample_device(pcm, 48000, 16000, device=gpu, channels=2, channel=2)
    with pytest.raises(DznError, match="beyond the output length 1600"):
        resample_device(x, 48000, 16000, device=gpu, out_range=(0, 1601))
    torch.cuda.synchronize()
    assert resample_device(x, 48000, 16000, device=gpu, out_range=(1599, 1600)).shape == (1,)


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def wav48(tmp_path_factory):
    """the 30 s fixture up-sampled to 48 kHz with the host resampler, as a PCM16 file"""
    from diarizen_amd.audio import first_channel_16k, resample
    x = resample(first_channel_16k(WAV), 16000, 48000)
    pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    body = pcm.tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 48000, 96000, 2, 16)
    p = tmp_path_factory.mktemp("resample") / "EN2002a_30s_48k.wav"
    p.write_bytes(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" +
                  struct.pack("<I", len(body)) + body)
    return str(p), pcm


@pytest.fixture(scope="module")
def pipe(gpu):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    p = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                         seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0), resample="device")
    yield p
    p.close()


def test_read_device_ranges_of_a_two_rank_split(built_lib, gpu, wav48, pipe):
    """ResampledSource.read_device(start, n) == slices of read_device(0, num_samples) for the sample ranges the two ranks of
    a sharded run take (dist.my_window_range's contiguous blocks: slice + halo), incl. the one that runs past the end"""
    from diarizen_amd.audio import ResampledSource
    from diarizen_amd.pipeline import open_recording, recording_on_device
    path, pcm = wav48
    src = open_recording(path, 16000, resample="device", device=gpu)
    assert isinstance(src, ResampledSource) and src.sample_rate == 16000
    assert src.num_samples == math.ceil(len(pcm) / 3)
    whole = src.read_device(0, src.num_samples)
    assert whole.shape == (src.num_samples,)
    r = pipe._runner
    C = r.num_windows(src.num_samples)
    assert C >= 4
    half = (C + 1) // 2
    for c0, c1 in ((0, half), (half, C)):
        lo, n = c0 * r.step, (c1 - c0 - 1) * r.step + r.window
        part = src.read_device(lo, n)
        assert torch.equal(part, whole[lo:lo + n])
        padded = recording_on_device(src, gpu, lo, n, zero_extend=True)      # what device_stage runs for that rank
        assert padded.shape == (n,)
        assert torch.equal(padded[:len(part)], part) and not padded[len(part):].any()
    assert src.read_device(src.num_samples, 10).shape == (0,)


def test_device_stage_on_the_resampled_source(built_lib, gpu, wav48, pipe):
    """device_stage on open_recording(resample="device") == device_stage on the host copy of resample_device of the whole
    file: seg and emb bit-identical"""
    from diarizen_amd.audio import resample_device
    from diarizen_amd.pipeline import open_recording
    path, pcm = wav48
    src = open_recording(path, 16000, resample="device", device=gpu)
    seg, emb = pipe.device_stage(src)
    wave = resample_device(pcm, 48000, 16000, device=gpu).cpu().numpy()
    seg2, emb2 = pipe.device_stage(wave)
    assert seg.shape == seg2.shape and seg.any()
    assert np.array_equal(seg, seg2) and np.array_equal(emb, emb2)


def test_pipeline_with_device_resampling(built_lib, gpu, wav48, pipe):
    """DiariZenPipeline(resample="device")(48 kHz file) -> Annotation; resample="host" on that file and the call on the
    16 kHz fixture give what they give without the feature (host waveform through device_stage + host_stage)"""
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.core import Annotation
    path, pcm = wav48
    ann = pipe(path, sess_name="EN2002a")
    assert isinstance(ann, Annotation) and len(ann.labels()) >= 1
    assert pipe.timings["audio_s"] == math.ceil(len(pcm) / 3) / 16000
    try:
        pipe.resample = "host"
        for f in (path, WAV):
            want = pipe.host_stage(*pipe.device_stage(first_channel_16k(f)), "EN2002a").to_rttm()
            assert pipe(f, sess_name="EN2002a").to_rttm() == want
    finally:
        pipe.resample = "device"
    assert pipe(WAV, sess_name="EN2002a").to_rttm() == want          # a 16 kHz file: "device" resamples nothing


def test_detection_with_device_resampling(built_lib, gpu, wav48, pipe):
    """the detection pipelines take the keyword (default: the DiariZenPipeline's) and read the source on the device"""
    from diarizen_amd.core import Annotation
    from diarizen_amd.detection import VoiceActivityDetection
    path, _ = wav48
    vad = VoiceActivityDetection(pipe)
    assert vad.resample == "device"
    speech = vad(path)
    assert isinstance(speech, Annotation) and speech.labels() == ["SPEECH"]
    assert VoiceActivityDetection(pipe, resample="host").resample == "host"
