"""Device decode in the resampler (csrc/resample.hip: src_format 2 .. 7 and the downmix, channel -1) on the MI355X.  Every
stored format must give the BITS of the float32 path (src_format 0, which this feature does not touch) on the host-decoded
channel or host downmix: the staging loop converts exactly, and the tap loop is the same code.  Then range calls, the
library's refusals and the plumbing up to the pipeline on an 8 kHz two-channel mu-law call, as WAV and as SPHERE."""
from __future__ import annotations

import audioop
import copy
import math
import os

import numpy as np
import pytest
import torch

from testkit.telephony import all_codes, sphere_bytes, wav_bytes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")

# (rate, T, channels): two full tiles of dzn_resample_tile() outputs plus a ragged third; o = 1 n = 2; o = 3 n = 1; even o
# (the padded LDS layout) with an odd channel count against the 3-byte format; o = 441 n = 640
SHAPES = [(8000, 1500, 2), (48000, 7200, 2), (32000, 5001, 3), (11025, 1700, 1)]


def _stored_forms(T: int, C: int, seed: int):
    """name -> (stored array, float32 [C, T] that the host decoders make of it), for every stored format"""
    from diarizen_amd.audio import alaw_table, ulaw_table
    g = np.random.default_rng(seed)
    forms = {}
    s16 = g.integers(-32768, 32768, size=(T, C)).astype(np.int16)
    forms["s16"] = (s16, s16.astype(np.float32) * np.float32(2.0 ** -15))
    u8 = g.integers(0, 256, size=(T, C)).astype(np.uint8)
    u8[:2, 0] = (0, 255)
    forms["u8"] = (u8, (u8.astype(np.float32) - 128.0) / 128.0)
    v24 = g.integers(-2 ** 23, 2 ** 23, size=(T, C)).astype(np.int32)
    v24[:2, 0] = (-2 ** 23, 2 ** 23 - 1)
    b24 = np.ascontiguousarray(v24.astype("<i4")[..., None].view(np.uint8)[..., :3]).reshape(T, 3 * C)
    forms["s24"] = (b24, v24.astype(np.float32) * np.float32(2.0 ** -23))
    s32 = g.integers(-2 ** 31, 2 ** 31, size=(T, C)).astype(np.int32)
    s32[:4, 0] = (-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3)      # round to even: up and down
    assert (s32.astype(np.float32).astype(np.float64) != s32).mean() > 0.9      # not representable in float32
    forms["s32"] = (s32, s32.astype(np.float32) * np.float32(2.0 ** -31))
    f32 = (0.3 * g.standard_normal((T, C))).astype(np.float32)
    forms["f32i"] = (f32, f32)
    for name, table in (("ulaw", ulaw_table()), ("alaw", alaw_table())):
        codes = all_codes(T, C, seed=seed + len(name))
        assert len(np.unique(codes)) == 256
        forms[name] = (codes, table[codes].astype(np.float32) * np.float32(2.0 ** -15))
    return {k: (stored, np.ascontiguousarray(dec.T)) for k, (stored, dec) in forms.items()}


@pytest.mark.parametrize("rate,T,C", SHAPES)
def test_every_stored_format_equals_the_float_path(built_lib, gpu, rate, T, C):
    """resample_device(stored, src_format=, channels=C, channel=c) is torch.equal to resample_device(host-decoded float32
    of channel c), and channel "downmix" (-1) to the one on audio.downmix of the decoded channels: codes 2 .. 7 and code 1"""
    from diarizen_amd.audio import downmix, resample_device, resample_tile, resampled_length, resample_bank
    _, o, n, _ = resample_bank(rate, 16000)
    M = resampled_length(T, o, n)
    assert 2 * resample_tile() < M < 3 * resample_tile() and M % resample_tile()
    for name, (stored, dec) in _stored_forms(T, C, seed=rate + T).items():
        for c in list(range(C)) + ["downmix", -1]:
            host = downmix(dec) if c in ("downmix", -1) else dec[c]
            want = resample_device(host, rate, 16000, device=gpu)                  # src_format 0
            got = resample_device(stored, rate, 16000, device=gpu, channels=C, channel=c, src_format=name)
            assert got.shape == (M,) and torch.equal(got, want), (name, c)
            if name in ("s16", "ulaw"):      # a device tensor as input gives the same bits as the host array
                dev = torch.from_numpy(stored.reshape(-1)).to(gpu)
                assert torch.equal(resample_device(dev, rate, 16000, device=gpu, channels=C, channel=c, src_format=name), want)
    # the code is inferred for int16, and the integer codes of dzn.h are taken as they are
    s16, dec = _stored_forms(T, C, seed=rate + T)["s16"]
    assert torch.equal(resample_device(s16, rate, 16000, device=gpu, channels=C, channel="downmix"),
                       resample_device(s16, rate, 16000, device=gpu, channels=C, channel=-1, src_format=1))


def test_range_calls_on_stored_mulaw(built_lib, gpu):
    """mu-law stereo at 8 kHz: a range call given only resample_input_span of the stored frames (first_index > 0 wherever
    the range does not start at the recording's start) == the slice of the whole call, bit for bit"""
    from diarizen_amd.audio import resample_bank, resample_device, resample_input_span, resample_tile
    rate, T, C = SHAPES[0]
    tile = resample_tile()
    _, o, n, width = resample_bank(rate, 16000)
    M = math.ceil(n * T / o)
    codes = all_codes(T, C, seed=77)
    for c in (0, 1, "downmix"):
        whole = resample_device(codes, rate, 16000, device=gpu, channels=C, channel=c, src_format="ulaw")
        assert whole.shape == (M,)
        for m0, m1 in ((0, 1), (tile - 1, tile + 1), (tile, 2 * tile), (M - 1, M)):
            lo, hi = resample_input_span(m0, m1, o, n, width)
            lo, hi = max(lo, 0), min(hi, T)
            assert lo > 0 or m0 == 0
            part = resample_device(codes[lo:hi], rate, 16000, device=gpu, out_range=(m0, m1), total=T, first_index=lo,
                                   channels=C, channel=c, src_format="ulaw")
            assert part.shape == (m1 - m0,) and torch.equal(part, whole[m0:m1]), (c, m0, m1)


def test_refusals(built_lib, gpu):
    """format 8, code 0 with two channels, channel -2 and channel == channels raise DznError with the library's message, and
    nothing is launched: a following valid call still returns"""
    from diarizen_amd._lib import DznError
    from diarizen_amd.audio import resample_device
    rate, T, C = SHAPES[0]
    codes = all_codes(T, C, seed=3)
    f32 = np.zeros((T, C), dtype=np.float32)
    with pytest.raises(DznError, match="src_format 8"):
        resample_device(codes, rate, 16000, device=gpu, channels=C, src_format=8)
    with pytest.raises(DznError, match="src_format 0 is float32 mono"):
        resample_device(f32, rate, 16000, device=gpu, channels=C, src_format=0)
    with pytest.raises(DznError, match="channel -2 of a source with 2 channel"):
        resample_device(codes, rate, 16000, device=gpu, channels=C, channel=-2, src_format="ulaw")
    with pytest.raises(DznError, match="channel 2 of a source with 2 channel"):
        resample_device(codes, rate, 16000, device=gpu, channels=C, channel=2, src_format="ulaw")
    with pytest.raises(ValueError, match="uint8 input needs src_format"):
        resample_device(codes, rate, 16000, device=gpu, channels=C)
    torch.cuda.synchronize()
    assert resample_device(codes, rate, 16000, device=gpu, channels=C, channel=1, src_format="ulaw").shape == (2 * T,)


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def call(tmp_path_factory):
    """the 30 s fixture as an 8 kHz two-channel mu-law call (channel 1 = channel 0 delayed by 0.5 s), as WAV and as SPHERE;
    -> (wav path, sphere path, decoded float32 [2, N])"""
    from diarizen_amd.audio import first_channel_16k, resample, ulaw_table
    x8 = resample(first_channel_16k(WAV), 16000, 8000)
    x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)      # [N, 2]
    pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    codes = np.frombuffer(audioop.lin2ulaw(pcm.tobytes(), 2), dtype=np.uint8).reshape(-1, 2)
    d = tmp_path_factory.mktemp("telephony")
    (d / "call.wav").write_bytes(wav_bytes(7, 2, 8000, 8, codes.tobytes()))
    (d / "call.sph").write_bytes(sphere_bytes("ulaw", 2, 8000, 1, codes.tobytes()))
    decoded = np.ascontiguousarray((ulaw_table()[codes].astype(np.float32) * np.float32(2.0 ** -15)).T)
    assert not np.array_equal(decoded[0], decoded[1])
    return str(d / "call.wav"), str(d / "call.sph"), decoded


@pytest.fixture(scope="module")
def pipe(gpu):
    """seeded weights as in tests/test_resample_gpu.py; built with channel=1 and resample="device\""""
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    p = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                         seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0), resample="device", channel=1)
    yield p
    p.close()


def test_open_recording_on_the_device(built_lib, gpu, call, pipe):
    """open_recording(resample="device", channel=c) of the WAV and the SPHERE file: a ResampledSource of the right length
    whose read_device ranges for a two-rank split equal slices of the whole, which is resample_device of the decoded choice"""
    from diarizen_amd.audio import ResampledSource, downmix, resample_device
    from diarizen_amd.pipeline import open_recording
    wav, sph, x = call
    r = pipe._runner
    for c in (0, 1, "downmix"):
        want = resample_device(downmix(x) if c == "downmix" else x[c], 8000, 16000, device=gpu)
        for path in (wav, sph):
            src = open_recording(path, 16000, resample="device", device=gpu, channel=c)
            assert isinstance(src, ResampledSource) and src.sample_rate == 16000 and src.num_samples == 2 * x.shape[1]
            whole = src.read_device(0, src.num_samples)
            assert torch.equal(whole, want), (path, c)
            W = r.num_windows(src.num_samples)
            half = (W + 1) // 2
            for c0, c1 in ((0, half), (half, W)):
                lo, n = c0 * r.step, (c1 - c0 - 1) * r.step + r.window
                assert torch.equal(src.read_device(lo, n), whole[lo:lo + n]), (path, c, c0)


def test_device_stage_on_the_call(built_lib, gpu, call, pipe):
    """device_stage(source) == device_stage(resample_device(host-decoded channel).cpu()) in seg and emb, bit for bit, for
    every channel choice; WAV and SPHERE of the same payload give identical seg and emb"""
    from diarizen_amd.audio import downmix, resample_device
    from diarizen_amd.pipeline import open_recording
    wav, sph, x = call
    for c in (0, 1, "downmix"):
        host = downmix(x) if c == "downmix" else x[c]
        seg0, emb0 = pipe.device_stage(resample_device(host, 8000, 16000, device=gpu).cpu().numpy())
        assert seg0.any()
        for path in (wav, sph):
            seg, emb = pipe.device_stage(open_recording(path, 16000, resample="device", device=gpu, channel=c))
            assert seg.shape == seg0.shape and np.array_equal(seg, seg0) and np.array_equal(emb, emb0), (path, c)


def test_pipeline_and_detection_take_the_channel(built_lib, gpu, call, pipe):
    """pipe(path) with channel="downmix" -> Annotation; {"audio": path, "channel": 1} on a channel-0 pipeline gives the RTTM
    of the pipeline built with channel=1; VoiceActivityDetection(pipe) inherits the channel; bad values are refused"""
    from diarizen_amd.core import Annotation
    from diarizen_amd.detection import VoiceActivityDetection
    from diarizen_amd.pipeline import DiariZenPipeline
    wav, sph, _ = call
    assert pipe.channel == 1
    want = pipe(sph, sess_name="call").to_rttm()                              # built with channel=1
    try:
        pipe.channel = "downmix"
        ann = pipe(sph, sess_name="call")
        assert isinstance(ann, Annotation) and len(ann.labels()) >= 1
        pipe.channel = 0
        rttm0 = pipe(sph, sess_name="call").to_rttm()
        assert pipe({"audio": sph, "channel": 1}, sess_name="call").to_rttm() == want
        assert pipe({"audio": wav, "channel": 1}, sess_name="call").to_rttm() == want
        assert pipe({"audio": sph}, sess_name="call").to_rttm() == rttm0
    finally:
        pipe.channel = 1
    vad = VoiceActivityDetection(pipe)
    assert vad.channel == 1 and vad.resample == "device"
    speech = vad(sph)
    assert isinstance(speech, Annotation) and speech.labels() == ["SPEECH"]
    assert VoiceActivityDetection(pipe, channel="downmix").channel == "downmix"
    for bad in (True, "left", -1):
        with pytest.raises(ValueError, match="channel"):
            VoiceActivityDetection(pipe, channel=bad)
        with pytest.raises(ValueError, match="channel"):
            DiariZenPipeline(None, None, config={"inference": {"args": {}}, "clustering": {"args": {}}}, channel=bad)
