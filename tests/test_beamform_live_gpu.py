"""Live array feeds on the MI355X (csrc/beamform_live.hip, streaming.WaveIngest): the one-pass planar decode
against dzn_decode channel by channel, the device delay tracker against the plain-loop rule in every partition, and the ingest
driven with the signals P, Q, R of testkit/beamform_live_ref.py in three chunkings — the device buffer must hold, bit for bit,
the float32 restatement of delay-and-sum with the reference causal delays AND what the offline BeamformedSource gives for the
same Beamform(causal=True), at one rate and through the resampler.  tests/test_beamform_live_host.py shows that no entry of
P, Q, R is within the comparison margin of a decision, so nothing is left out here.  Then the sessions: pipeline.stream,
open_live and the detection stream on a 4-microphone int16 feed give what the offline pipeline gives on the same WAV."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest
import torch

from _stream_cases import FEED, RECORDINGS, feeds, samples
from testkit import beamform_live_ref as LR
from testkit import beamform_ref as R
from testkit.telephony import wav_bytes

pytestmark = pytest.mark.gpu

PACKET = 5921
SRC = {"f32": 0, "s16": 1, "u8": 2, "s24": 3, "s32": 4, "f32i": 5, "ulaw": 6, "alaw": 7}
STORED = {0: (np.float32, 1), 1: (np.int16, 1), 2: (np.uint8, 1), 3: (np.uint8, 3), 4: (np.int32, 1), 5: (np.float32, 1),
          6: (np.uint8, 1), 7: (np.uint8, 1)}      # stored dtype, elements per sample


def _stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


# ----------------------------------------------------------------------------- dzn_decode_planar
def _stored(fmt: int, frames: int, channels: int, seed: int):
    g = np.random.default_rng(seed)
    dtype, per = STORED[fmt]
    n = frames * channels * per
    if dtype == np.float32:
        return g.standard_normal(n).astype(np.float32)
    info = np.iinfo(dtype)
    return g.integers(info.min, info.max + 1, size=n, dtype=np.int64).astype(dtype)


@pytest.mark.parametrize("name", sorted(SRC, key=SRC.get))
def test_decode_planar_equals_decode_channel_by_channel(built_lib, gpu, name):
    lib, fmt = built_lib, SRC[name]
    for channels in ((1,) if fmt == 0 else (2, 3, 8)):
        for frames in (1, 255, 256, 1025):
            src = torch.from_numpy(_stored(fmt, frames, channels, 31 * frames + channels)).to(gpu)
            stride = frames + 7
            got = torch.full((channels, stride), -7.0, device=gpu, dtype=torch.float32)
            assert lib.dzn_decode_planar(gpu.index, _ptr(src), fmt, channels, frames, _ptr(got), stride, _stream(gpu)) == 0
            want = torch.empty((channels, frames), device=gpu, dtype=torch.float32)
            for c in range(channels):
                assert lib.dzn_decode(gpu.index, _ptr(src), fmt, channels, c, frames, _ptr(want[c]), _stream(gpu)) == 0
            assert torch.equal(got[:, :frames], want), (name, channels, frames)
            assert (got[:, frames:] == -7.0).all(), (name, channels, frames)      # the padding of a row is not touched
            assert want.abs().max() > 0


def test_decode_planar_refusals(built_lib, gpu):
    lib = built_lib
    src = torch.zeros(64, device=gpu, dtype=torch.int16)
    dst = torch.zeros((2, 16), device=gpu, dtype=torch.float32)

    def call(fmt=1, channels=2, frames=16, stride=16, off=0, d=dst):
        rc = lib.dzn_decode_planar(gpu.index, _ptr(src, off), fmt, channels, frames, _ptr(d) if d is not None else None, stride,
                                   _stream(gpu))
        return rc, lib.dzn_last_error(None).decode()

    assert call()[0] == 0 and call(frames=0)[0] == 0
    for kw, why in ((dict(fmt=8), "src_format 8"), (dict(fmt=-1), "src_format -1"), (dict(channels=0), "0 channel"),
                    (dict(fmt=0), "float32 mono"), (dict(frames=-1), "bad frames"), (dict(stride=15), "ch_stride"),
                    (dict(off=1), "not aligned"), (dict(fmt=4, off=2), "not aligned"), (dict(d=None), "null pointer")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("dzn_decode_planar: ") and why in msg, (kw, rc, msg)
    torch.cuda.synchronize(gpu)
    assert not dst.any()                                                # a refused call launches nothing


# ----------------------------------------------------------------------------- dzn_beamform_track
def _track(lib, gpu, lag, peak, T, hop, min_peak, parts, ref=0):
    """the table and the final state of tracking the blocks in the consecutive ranges `parts`"""
    Cn, nb = lag.shape
    d_lag = torch.from_numpy(np.array(lag, dtype=np.int32, order="C")).to(gpu)       # (row-major copies: the reference's are not)
    d_peak = torch.from_numpy(np.array(peak, dtype=np.float32, order="C")).to(gpu)
    state = torch.zeros((Cn, 5), device=gpu, dtype=torch.int32)
    table = torch.full((Cn, nb + 3), 99, device=gpu, dtype=torch.int32)
    seen = C.c_int64(0)
    for b0, b1 in parts:
        # rows of stride nb whose column 0 is block b0
        rc = lib.dzn_beamform_track(gpu.index, _ptr(d_lag, 4 * b0), _ptr(d_peak, 4 * b0), nb, Cn, ref, hop, T, min_peak, b0, b1,
                                    _ptr(state), C.byref(seen), _ptr(table), nb + 3, _stream(gpu))
        assert rc == 0 and seen.value == b1, lib.dzn_last_error(None)
    out = table.cpu().numpy()
    assert (out[:, nb:] == 99).all()
    return out[:, :nb], state.cpu().numpy()


def _track_cases():
    lag, peak, T, hop, min_peak = LR.random_case()
    yield "random", lag, peak, T, hop, min_peak
    c = LR.signal("P")
    lag, peak, _ = LR.reference("P")
    yield "P", lag, peak.astype(np.float32), c["T"], c["hop"], c["min_peak"]


def test_track_equals_the_rule_in_every_partition(built_lib, gpu):
    for name, lag, peak, T, hop, min_peak in _track_cases():
        nb = lag.shape[1]
        want = LR.causal_delays(lag, peak, T, hop, min_peak, 0)
        whole, state = _track(built_lib, gpu, lag, peak, T, hop, min_peak, [(0, nb)])
        assert np.array_equal(whole, want), name
        assert state[:, 4].tolist() == [nb] * lag.shape[0]
        for parts in ([(b, b + 1) for b in range(nb)], [(0, 1), (1, 7), (7, nb)]):
            table, st = _track(built_lib, gpu, lag, peak, T, hop, min_peak, parts)
            assert np.array_equal(table, want) and np.array_equal(st, state), (name, parts)
    lag, peak, T, hop, min_peak = LR.random_case()
    assert np.array_equal(_track(built_lib, gpu, lag, peak, T, hop, min_peak, [(0, 23)], ref=2)[0],
                          LR.causal_delays(lag, peak, T, hop, min_peak, 2))


def test_track_refuses_a_block_out_of_sequence(built_lib, gpu):
    lib = built_lib
    lag, peak, T, hop, min_peak = LR.random_case()
    d_lag, d_peak = torch.from_numpy(lag).to(gpu), torch.from_numpy(peak).to(gpu)
    state = torch.zeros((4, 5), device=gpu, dtype=torch.int32)
    table = torch.zeros((4, 23), device=gpu, dtype=torch.int32)
    seen = C.c_int64(0)

    def call(b0, b1, channels=4, ref=0, h=hop, stride=23, nblk=23):
        rc = lib.dzn_beamform_track(gpu.index, _ptr(d_lag), _ptr(d_peak), nblk, channels, ref, h, T, min_peak, b0, b1, _ptr(state),
                                    C.byref(seen), _ptr(table), stride, _stream(gpu))
        return rc, lib.dzn_last_error(None).decode()

    assert call(0, 3)[0] == 0 and seen.value == 3
    for b0 in (0, 2, 4):
        rc, msg = call(b0, 5)
        assert rc == -1 and "out of sequence" in msg and seen.value == 3, (b0, msg)
    for kw, why in ((dict(channels=1), "1 channel"), (dict(channels=65), "65 channel"), (dict(ref=4), "reference channel 4"),
                    (dict(h=300), "hop 300"), (dict(stride=4), "do not fit"), (dict(nblk=1), "do not fit")):
        rc, msg = call(3, 5, **kw)
        assert rc == -1 and msg.startswith("dzn_beamform_track: ") and why in msg, (kw, msg)
    rc, msg = call(3, 24)
    assert rc == -1 and "are not inside the 23 blocks" in msg
    assert call(3, 3)[0] == 0 and call(3, 23)[0] == 0 and seen.value == 23


# ----------------------------------------------------------------------------- the ingest
def _bf(c, rate=16000):
    from diarizen_amd.audio import Beamform
    return Beamform(causal=True, hop=c["hop"], max_delay=c["max_lag"] / rate)


_OFFLINE: dict = {}


def _offline(gpu, name, x, bf, rate):
    """BeamformedSource of the whole array at 16 kHz, read once per (signal, feed rate): (samples, delays)"""
    from diarizen_amd.audio import BeamformedSource
    if (name, rate) not in _OFFLINE:
        src = BeamformedSource(x, 16000, gpu, bf, orig_rate=rate)
        _OFFLINE[name, rate] = (src.read_device(0, src.num_samples), src.delays)
    return _OFFLINE[name, rate]


def _chunkings(raw: bytes, hop: int, frame_bytes: int):
    """(chunks, slot_frames): one chunk, 5921-byte packets (which end inside a frame), and chunks of 2 hop - 1 frames into
    slots of hop frames, so that every chunk is split"""
    step = (2 * hop - 1) * frame_bytes
    yield [raw], None
    yield [raw[i:i + PACKET] for i in range(0, len(raw), PACKET)], None
    yield [raw[i:i + step] for i in range(0, len(raw), step)], hop


def _ingest(gpu, fmt, slot_frames, max_seconds=1.0):
    from diarizen_amd.streaming import WaveIngest
    return WaveIngest(gpu, 16000, 1600, 160, max_seconds=max_seconds, slot_seconds=1.0, slots=3, feed_format=fmt,
                      slot_frames=slot_frames)


@pytest.mark.parametrize("name", ["P", "Q", "R"])
def test_ingest_equals_the_restatement_and_the_offline_source(built_lib, gpu, name):
    from diarizen_amd.audio import FeedFormat
    c = LR.signal(name)
    x, T, hop = c["x"], c["T"], c["hop"]
    bf = _bf(c)
    fmt = FeedFormat(16000, "s16", channels=4, channel=bf)
    assert bf.plan(16000, 4) == (hop, c["max_lag"], c["min_peak"])
    want_d = LR.reference_delays(name)
    want = torch.from_numpy(R.synth(x, want_d, hop)).to(gpu)
    offline, offline_d = _offline(gpu, name, x, bf, 16000)
    assert np.array_equal(offline_d, want_d) and torch.equal(offline, want)
    raw = LR.frames_of(x).tobytes()
    for chunks, slot_frames in _chunkings(raw, hop, fmt.frame_bytes):
        ing = _ingest(gpu, fmt, slot_frames)
        for ch in chunks:
            ing.append(ch)
            assert ing.n == LR.beam_ready(ing.frames, hop)
        assert ing.frames == T and ing.n < T
        assert ing.flush() == T - LR.beam_ready(T, hop) and ing.n == T and ing.flush() == 0
        ing.wait()
        assert torch.equal(ing.dev_wave[:T], want), (name, slot_frames, len(chunks))
        assert not ing.dev_wave[T:].any()                               # nothing is written behind the recording
        assert np.array_equal(ing.delays(), want_d)
        if slot_frames is not None:
            assert ing.uploads > len(chunks)                            # the chunks were split


def test_ingest_short_empty_and_silent_streams(built_lib, gpu):
    from diarizen_amd.audio import FeedFormat
    c = LR.signal("P")
    bf = _bf(c)
    fmt = FeedFormat(16000, "s16", channels=4, channel=bf)
    x = c["x"][:, :100]
    ing = _ingest(gpu, fmt, None)
    assert ing.append(LR.frames_of(x).tobytes()) == 0 and ing.flush() == 100 and ing.n == ing.frames == 100
    ing.wait()
    zero = np.zeros((4, 2), dtype=np.int32)
    assert np.array_equal(ing.delays(), zero)                           # no block of 100 samples is supported
    assert torch.equal(ing.dev_wave[:100], torch.from_numpy(R.synth(x, zero, 256)).to(gpu)) and ing.dev_wave[:100].any()
    assert torch.equal(ing.dev_wave[:100], _offline(gpu, "P100", x, bf, 16000)[0]) and not ing.dev_wave[100:].any()
    ing = _ingest(gpu, fmt, None)                                       # an empty stream
    assert ing.append(b"") == 0 and ing.flush() == 0 and ing.n == 0
    ing.wait()
    assert not ing.dev_wave.any() and np.array_equal(ing.delays(), np.zeros((4, 1), dtype=np.int32))
    # silent microphones beside the reference: every block has peak 0, the delays stay 0 throughout
    x = np.array(c["x"])
    x[1:] = 0
    ing = _ingest(gpu, fmt, 256)
    for ch in packets(LR.frames_of(x).tobytes()):
        ing.append(ch)
    ing.flush()
    ing.wait()
    d = ing.delays()
    assert d.shape == (4, R.num_blocks(c["T"], 256)) and not d.any()
    assert torch.equal(ing.dev_wave[:c["T"]], torch.from_numpy(R.synth(x, d, 256)).to(gpu))


def test_ingest_at_another_rate_equals_the_offline_source(built_lib, gpu):
    """R as a 48 kHz feed into a 16 kHz ingest: beamformed at 48 kHz, then the device resampler, as the offline source does"""
    from diarizen_amd.audio import FeedFormat, resampled_length
    c = LR.signal("R")
    x, T, hop = c["x"], c["T"], c["hop"]
    bf = _bf(c, 48000)
    assert bf.plan(48000, 4) == (hop, c["max_lag"], c["min_peak"])
    fmt = FeedFormat(48000, "s16", channels=4, channel=bf)
    want, want_d = _offline(gpu, "R", x, bf, 48000)
    N = resampled_length(T, 3, 1)
    assert len(want) == N and np.array_equal(want_d, LR.reference_delays("R")) and want.any()
    raw = LR.frames_of(x).tobytes()
    for chunks, slot_frames in _chunkings(raw, hop, fmt.frame_bytes):
        ing = _ingest(gpu, fmt, slot_frames)
        n = 0
        for ch in chunks:
            ing.append(ch)
            assert n <= ing.n <= resampled_length(LR.beam_ready(ing.frames, hop), 3, 1)
            n = ing.n
        ing.flush()
        ing.wait()
        assert ing.n == N and ing.frames == T
        assert torch.equal(ing.dev_wave[:N], want), (slot_frames, len(chunks))
        assert not ing.dev_wave[N:].any() and np.array_equal(ing.delays(), want_d)


# ----------------------------------------------------------------------------- sessions
DELAYS = (0, 5, -12, 30)


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    """the seeded-weights pipeline of tests/test_feed_sessions_gpu.py, with channel=Beamform(causal=True)"""
    from diarizen_amd.audio import Beamform
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    p = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                         seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0), resample="device",
                         channel=Beamform(causal=True))
    yield p
    p.close()


@pytest.fixture(scope="module")
def arrays(tmp_path_factory):
    """name -> (wav path, the feed's bytes, frames, float32 [4, N]): the recording on four microphones at 16 kHz — delayed
    copies plus noise — as int16 frames, and the same frames as a WAV file"""
    d = tmp_path_factory.mktemp("arrays")
    out = {}
    for name in ("grid", "short"):
        s = samples(RECORDINGS[name])[0]
        x = R.delayed_copies(s, DELAYS, 0.002, 17)
        pcm = np.clip(np.rint(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")      # [N, 4]
        body = pcm.tobytes()
        assert len(body) % PACKET and PACKET % 8
        (d / f"{name}.wav").write_bytes(wav_bytes(1, 4, 16000, 16, body))
        out[name] = (str(d / f"{name}.wav"), body, len(pcm), np.ascontiguousarray(pcm.T.astype(np.float32) * np.float32(2.0 ** -15)))
    return out


def packets(body: bytes):
    return [body[i:i + PACKET] for i in range(0, len(body), PACKET)]


def feed_format(channel=None):
    from diarizen_amd.audio import FeedFormat
    return FeedFormat(16000, "s16", channels=4, channel=channel)


def crop(ann, t: float):
    return sorted((seg.start, min(seg.end, t), lab) for seg, _, lab in ann.itertracks(yield_label=True) if seg.start < t)


@pytest.mark.parametrize("name", ["grid", "short"])
def test_stream_gives_the_offline_rttm(pipe, gpu, arrays, name):
    from diarizen_amd.audio import BeamformedSource
    from diarizen_amd.pipeline import open_recording
    from diarizen_amd.streaming import StreamingSession
    wav, body, frames, _ = arrays[name]
    want = pipe(wav, sess_name=name).to_rttm()
    assert want or name == "short"
    out = list(pipe.stream(packets(body), sess_name=name, feed_format=feed_format(), max_seconds=60.0, slot_seconds=2.5, slots=3))
    secs, ann = out[-1]
    assert secs == frames / 16000 and ann.to_rttm() == want
    seg0, emb0 = pipe.device_stage(open_recording(wav, 16000, resample="device", device=gpu, channel=pipe.channel))
    sess = StreamingSession(pipe, name, max_seconds=60.0, refresh_s=None, feed_format=feed_format(pipe.channel))
    assert all(sess.feed(p) is None for p in packets(body)) and sess.ingest.frames == frames
    assert sess.finish().to_rttm() == want and sess.n == frames
    assert (seg0.any() or name == "short") and np.array_equal(np.concatenate(sess.seg), seg0)
    assert np.array_equal(np.concatenate(sess.emb), emb0)
    twin = BeamformedSource(arrays[name][3], 16000, gpu, pipe.channel, orig_rate=16000)
    assert np.array_equal(sess.ingest.delays(), twin.estimate()) and twin.delays.any()      # the offline twin's table


@pytest.mark.parametrize("name", ["grid", "short"])
def test_open_live_equals_the_float32_session(pipe, gpu, arrays, name):
    from diarizen_amd.audio import BeamformedSource, beam_ready
    wav, body, frames, x = arrays[name]
    src = BeamformedSource(x, 16000, gpu, pipe.channel, orig_rate=16000)
    whole = src.read_device(0, frames).cpu().numpy()
    ref = pipe.open_live(sess_name=name, max_seconds=60.0)
    for chunk in feeds(whole, FEED):
        ref.feed(chunk)
    ref_ann = ref.finish()
    sess = pipe.open_live(sess_name=name, max_seconds=60.0, slot_seconds=2.5, slots=3, feed_format=feed_format())
    for p in packets(body):
        sess.feed(p)
        assert sess.n == beam_ready(sess.ingest.frames, src.hop)
    ann = sess.finish()
    assert sess.n == ref.n == frames and sess.done == ref.done > 0
    assert torch.equal(sess.ingest.dev_wave[:frames].cpu(), torch.from_numpy(whole))
    assert np.array_equal(sess.committed_diarization, ref.committed_diarization)
    assert np.array_equal(sess.hard_clusters, ref.hard_clusters)
    assert ann.to_rttm() == ref_ann.to_rttm()


@pytest.mark.parametrize("name", ["grid", "short"])
def test_detection_stream_final_and_committed_prefixes(pipe, gpu, arrays, name):
    from diarizen_amd.detection import VoiceActivityDetection
    wav, body, frames, _ = arrays[name]
    vad = VoiceActivityDetection(pipe)
    want = vad({"audio": wav, "uri": name})
    out = list(vad.stream(packets(body), uri=name, feed_format=feed_format(), max_seconds=60.0, slot_seconds=2.5, slots=3))
    secs, committed, final = out[-1]
    assert secs == frames / 16000 and final.to_rttm() == want.to_rttm()
    assert want.to_rttm() or name == "short"
    for s, t, ann in out[:-1]:
        assert t <= s <= secs and crop(ann, t) == crop(final, t)


def test_refused_when_the_session_opens(pipe, gpu):
    from diarizen_amd.audio import Beamform, FeedFormat
    from diarizen_amd.detection import VoiceActivityDetection
    offline_only = copy.copy(pipe)                                       # the same engine with the non-causal channel choice
    offline_only.channel = Beamform()
    for open_ in (lambda: offline_only.open_live(feed_format=feed_format()),
                  lambda: next(offline_only.stream([b""], feed_format=feed_format())),
                  lambda: VoiceActivityDetection(offline_only).open_stream(feed_format=feed_format()),
                  lambda: pipe.open_live(feed_format=feed_format(Beamform()))):
        with pytest.raises(ValueError, match=r"pass Beamform\(causal=True\)"):
            open_()
    with pytest.raises(ValueError, match="1 channel"):
        pipe.open_live(feed_format=FeedFormat(16000, "s16"))             # a mono feed is no array
    hub = pipe.open_hub(max_sessions=1, max_seconds=10.0)
    with pytest.raises(ValueError, match="array feed"):
        hub.open("room", feed_format=feed_format())
    assert hub.open("room", feed_format=feed_format(0)) is not None      # the row was not taken by the refusal
    hub.close()
