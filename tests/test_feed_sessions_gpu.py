"""Sessions fed in a stored format (feed_format=audio.FeedFormat) on the MI355X: the recordings of tests/_stream_cases.py as
8 kHz two-channel mu-law calls, fed in 5921-byte packets (which end inside a frame), must give what the offline pipeline
gives on the same call as a WAV file with resample="device" — pipeline.stream, the detection pipelines' stream and
pipeline.open_live — and a 16 kHz int16 feed what the float32 session gives."""
from __future__ import annotations

import audioop
import copy

import numpy as np
import pytest
import torch

from _stream_cases import FEED, RECORDINGS, feeds, samples
from testkit.telephony import wav_bytes

pytestmark = pytest.mark.gpu

PACKET = 5921
CASES = [(name, c) for name in ("grid", "short") for c in (1, "downmix")]


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    """the seeded-weights pipeline of tests/test_telephony_gpu.py: resample="device", channel=1, 8 s windows"""
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    p = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                         seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0), resample="device", channel=1)
    yield p
    p.close()


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    """name -> (wav path, the call's bytes, frames): the recording as an 8 kHz two-channel mu-law call (channel 1 = channel 0
    delayed by 0.5 s), as the `call` fixture of tests/test_telephony_gpu.py makes it"""
    from diarizen_amd.audio import resample
    d = tmp_path_factory.mktemp("feeds")
    out = {}
    for name in ("grid", "short"):
        x8 = resample(samples(RECORDINGS[name])[0], 16000, 8000)
        x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)      # [N, 2]
        pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
        body = audioop.lin2ulaw(pcm.tobytes(), 2)
        assert len(body) == 2 * {"grid": 128000, "short": 40000}[name] and len(body) % PACKET and PACKET % 2
        (d / f"{name}.wav").write_bytes(wav_bytes(7, 2, 8000, 8, body))
        out[name] = (str(d / f"{name}.wav"), body, len(body) // 2)
    return out


def packets(body: bytes):
    return [body[i:i + PACKET] for i in range(0, len(body), PACKET)]


def fmt(channel=None):
    from diarizen_amd.audio import FeedFormat
    return FeedFormat(8000, "ulaw", channels=2, channel=channel)


def crop(ann, t: float):
    """the turns of an annotation before time t, cut at t"""
    return sorted((seg.start, min(seg.end, t), lab) for seg, _, lab in ann.itertracks(yield_label=True) if seg.start < t)


@pytest.mark.parametrize("name,c", CASES)
def test_stream_gives_the_offline_rttm(pipe, gpu, calls, name, c):
    wav, body, frames = calls[name]
    want = pipe({"audio": wav, "channel": c}, sess_name=name).to_rttm()
    assert want or name == "short"                                      # (5 s of the seeded model: no turns, offline either)
    out = list(pipe.stream(packets(body), sess_name=name, feed_format=fmt(c), max_seconds=60.0, slot_seconds=2.5, slots=3))
    secs, ann = out[-1]
    assert secs == 2 * frames / 16000 and ann.to_rttm() == want
    assert [t for t, _ in out] == sorted(t for t, _ in out)
    if c == 1:                                                          # a format without a channel takes the pipeline's
        assert pipe.channel == 1
        assert list(pipe.stream(packets(body), sess_name=name, feed_format=fmt(), max_seconds=60.0))[-1][1].to_rttm() == want
    # the push form, and what the windows gave before the host stage: the offline device stage of the file, bit for bit
    from diarizen_amd.pipeline import open_recording
    from diarizen_amd.streaming import StreamingSession
    seg0, emb0 = pipe.device_stage(open_recording(wav, 16000, resample="device", device=gpu, channel=c))
    sess = StreamingSession(pipe, name, max_seconds=60.0, refresh_s=None, feed_format=fmt(c))
    assert all(sess.feed(p) is None for p in packets(body)) and sess.ingest.frames == frames
    assert sess.finish().to_rttm() == want and sess.n == 2 * frames
    assert (seg0.any() or name == "short") and np.array_equal(np.concatenate(sess.seg), seg0) and np.array_equal(np.concatenate(sess.emb), emb0)


@pytest.mark.parametrize("name,c", CASES)
def test_detection_stream_final_and_committed_prefixes(pipe, gpu, calls, name, c):
    from diarizen_amd.detection import VoiceActivityDetection
    wav, body, frames = calls[name]
    vad = VoiceActivityDetection(pipe, channel=c)
    want = vad({"audio": wav, "uri": name})
    out = list(vad.stream(packets(body), uri=name, feed_format=fmt(), max_seconds=60.0, slot_seconds=2.5, slots=3))
    secs, committed, final = out[-1]
    assert secs == 2 * frames / 16000 and final.to_rttm() == want.to_rttm()
    assert want.to_rttm() or name == "short"
    assert len(out) == 1 if name == "short" else len(out) > 10
    for s, t, ann in out[:-1]:
        assert t <= s <= secs and crop(ann, t) == crop(final, t)


@pytest.mark.parametrize("name,c", CASES)
def test_open_live_equals_the_float32_session(pipe, gpu, calls, name, c):
    from diarizen_amd.audio import resample_device
    wav, body, frames = calls[name]
    codes = np.frombuffer(body, dtype=np.uint8).reshape(-1, 2)
    whole = resample_device(codes, 8000, 16000, device=gpu, channels=2, channel=c, src_format="ulaw").cpu().numpy()
    ref = pipe.open_live(sess_name=name, max_seconds=60.0)
    for chunk in feeds(whole, FEED):
        ref.feed(chunk)
    ref_ann = ref.finish()
    sess = pipe.open_live(sess_name=name, max_seconds=60.0, slot_seconds=2.5, slots=3, feed_format=fmt(c))
    for p in packets(body):
        sess.feed(p)
        assert sess.ingest.frames <= frames and sess.n == max(0, sess.ingest.frames - 7) * 2      # audio.feed_ready: width 7, o 1, n 2
    ann = sess.finish()
    assert sess.n == ref.n == len(whole) and sess.done == ref.done > 0
    assert np.array_equal(sess.committed_diarization, ref.committed_diarization)
    assert np.array_equal(sess.committed_count, ref.committed_count)
    assert np.array_equal(sess.hard_clusters, ref.hard_clusters)
    assert ann.to_rttm() == ref_ann.to_rttm()
    with pytest.raises(RuntimeError):
        sess.feed(b"\0\0")


def test_int16_feed_at_the_model_rate(pipe, gpu):
    """16 kHz int16 mono of "short" (through dzn_decode): the float32 session's results exactly, and the offline RTTM of the
    WAV; arrays of the stored dtype are taken as well as bytes"""
    import io
    import wave
    from diarizen_amd.audio import FeedFormat
    x, data = samples(RECORDINGS["short"])
    with wave.open(io.BytesIO(data), "rb") as r:
        pcm = r.readframes(r.getnframes())
    want = pipe({"audio": data, "channel": 0}, sess_name="short").to_rttm()
    f32 = list(pipe.stream(feeds(x), sess_name="short", max_seconds=60.0))[-1][1].to_rttm()
    ff = FeedFormat(16000, "s16", channel=0)
    got = list(pipe.stream(packets(pcm), sess_name="short", feed_format=ff, max_seconds=60.0))
    assert got[-1][0] == len(x) / 16000 and got[-1][1].to_rttm() == f32 == want
    arrays = feeds(np.frombuffer(pcm, dtype=np.int16), FEED)
    assert list(pipe.stream(arrays, sess_name="short", feed_format=ff, max_seconds=60.0))[-1][1].to_rttm() == want
    from diarizen_amd.streaming import StreamingSession
    a, b = StreamingSession(pipe, "short", max_seconds=60.0), StreamingSession(pipe, "short", max_seconds=60.0, feed_format=ff)
    for u, v in zip(feeds(x), arrays):
        a.feed(u)
        b.feed(v)
        assert a.n == b.n == b.ingest.frames
    a.finish(), b.finish()
    assert torch.equal(a.ingest.dev_wave, b.ingest.dev_wave) and a.ingest.dev_wave[:80000].any()
    assert np.array_equal(np.concatenate(a.seg), np.concatenate(b.seg)) and np.array_equal(np.concatenate(a.emb), np.concatenate(b.emb))
    ref = pipe.open_live(sess_name="short", max_seconds=60.0)
    sess = pipe.open_live(sess_name="short", max_seconds=60.0, feed_format=ff)
    for a, b in zip(feeds(x), arrays):
        ref.feed(a)
        sess.feed(b)
    assert ref.finish().to_rttm() == sess.finish().to_rttm()
    assert np.array_equal(sess.committed_diarization, ref.committed_diarization)
    assert np.array_equal(sess.hard_clusters, ref.hard_clusters)


def test_refused_when_the_session_opens(pipe, gpu):
    from diarizen_amd.audio import FeedFormat
    from diarizen_amd.detection import VoiceActivityDetection
    with pytest.raises(ValueError, match="channel 1 of a source with 1 channel"):
        pipe.open_live(feed_format=FeedFormat(8000, "ulaw"))            # the pipeline's channel 1 on a mono feed
    with pytest.raises(ValueError, match="does not fit in LDS"):
        VoiceActivityDetection(pipe).open_stream(feed_format=FeedFormat(15999, "s16", channel=0))
    with pytest.raises(ValueError, match="FeedFormat"):
        next(pipe.stream([b""], feed_format="ulaw"))
    sess = pipe.open_live(max_seconds=10.0, feed_format=FeedFormat(8000, "s16", channel=0))
    with pytest.raises(ValueError, match="int16"):
        sess.feed(np.zeros(160, dtype=np.float32))
    assert sess.finish().to_rttm() == ""
