"""Array feeds in a live hub (diarizen_amd/hub.py, csrc/beamform_many.hip) on the MI355X: a 4-microphone
16 kHz array, a 4-microphone 48 kHz array and an ordinary mu-law call fed interleaved in unequal packets with one tick() per
round.  Every session must end with the waveform row, the delay table, the committed arrays, labels and RTTM of the same feed
through pipeline.open_live ALONE, bit for bit, while all array calls of a tick share one upload and one dzn_beamform_many; then
several waves in one tick, the reuse of a finished array session's row, the detection hub and the default hub's refusal."""
from __future__ import annotations

import audioop
import copy

import numpy as np
import pytest
import torch

from _stream_cases import RECORDINGS, samples
from testkit import beamform_ref as R

pytestmark = pytest.mark.gpu

DELTA = 0.2                                         # the seeded embedding weights: 3 speakers at 0.2
DELAYS = (0, 5, -12, 30)
PACKET16, PACKET48, PACKET_CALL = 65537, 99999, 5921      # bytes per feed: each ends inside a frame


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    """the seeded wavlm_large_s80_md pipeline of tests/test_hub_gpu.py: 8 s windows, batches of 64"""
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    p = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield p
    p.close()


def array_bytes(s, delays) -> bytes:
    """the recording on four microphones — delayed copies plus noise — as interleaved int16 frames (the `arrays` fixture of
    tests/test_beamform_live_gpu.py)"""
    x = R.delayed_copies(s, delays, 0.002, 17)
    return np.clip(np.rint(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()


def cut(body: bytes, size: int):
    assert len(body) % size and size % 8
    return [body[i:i + size] for i in range(0, len(body), size)]


@pytest.fixture(scope="module")
def sources():
    """name -> (feed_format, the chunks of its feed loop)"""
    from diarizen_amd.audio import Beamform, FeedFormat, resample
    bf = Beamform(causal=True)
    out = {"grid": (FeedFormat(16000, "s16", channels=4, channel=bf), cut(array_bytes(samples(RECORDINGS["grid"])[0], DELAYS), PACKET16))}
    short = samples(RECORDINGS["short"])[0]
    out["short16"] = (FeedFormat(16000, "s16", channels=4, channel=bf), cut(array_bytes(short, DELAYS), PACKET16))
    x48 = resample(short, 16000, 48000)
    out["short48"] = (FeedFormat(48000, "s16", channels=4, channel=bf), cut(array_bytes(x48, tuple(3 * d for d in DELAYS)), PACKET48))
    # the call of tests/test_hub_gpu.py: 8 kHz, two channels (channel 1 = channel 0 delayed by 0.5 s), mu-law
    x8 = resample(short, 16000, 8000)
    x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)
    body = audioop.lin2ulaw(np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes(), 2)
    out["call"] = (FeedFormat(8000, "ulaw", channels=2, channel=1), [body[i:i + PACKET_CALL] for i in range(0, len(body), PACKET_CALL)])
    assert len({len(out[k][1]) for k in ("grid", "short48", "call")}) == 3          # unequal chunking
    return out


def final_state(sess):
    return (sess.committed_diarization, sess.committed_count, sess.hard_clusters, sess.result.to_rttm())


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def delays_of(sess):
    return sess.ingest.delays() if sess.ingest.array else None


def run_solo(open_session, fmt, chunks):
    sess = open_session(fmt)
    for c in chunks:
        sess.feed(c)
    sess.finish()
    torch.cuda.synchronize()
    return sess


@pytest.fixture(scope="module")
def solo(pipe, sources, tmp_path_factory):
    """name -> (final state, dev_wave[:n], n, delays or None, RTTM file's text) of the session ALONE (pipeline.open_live)"""
    d = tmp_path_factory.mktemp("solo")
    pipe.rttm_out_dir = str(d)
    out = {}
    try:
        for name, (fmt, chunks) in sources.items():
            s = run_solo(lambda f: pipe.open_live(sess_name=name, delta_new=DELTA, max_seconds=60.0, feed_format=f), fmt, chunks)
            out[name] = (final_state(s), s.ingest.dev_wave[:s.n].clone(), s.n, delays_of(s), (d / f"{name}.rttm").read_text())
            del s
    finally:
        pipe.rttm_out_dir = None
    return out


def drive(hub, sessions, sources, after_tick=None, per_round=1):
    """feed round-robin, `per_round` chunks per session and round, finish() a session once its chunks are out, tick() after
    every round; -> the ticks' results"""
    todo = {name: list(sources[name][1]) for name in sessions}
    open_ = set(sessions)
    results = []
    while open_:
        for name in sorted(open_):
            if todo[name]:
                for _ in range(min(per_round, len(todo[name]))):
                    sessions[name].feed(todo[name].pop(0))
            else:
                assert sessions[name].finish() is None
                open_.discard(name)
        out = hub.tick()
        results.append(out)
        if after_tick is not None:
            after_tick(out)
    return results


def check_against_solo(s, want_all, name):
    want, wave, n, delays, _ = want_all
    assert s.finished and s.n == n
    assert torch.equal(s.ingest.dev_wave[:n], wave), name                              # the pool row is the solo waveform
    assert bool((s.ingest.dev_wave[n:] == 0).all())
    if delays is not None:
        got = s.ingest.delays()
        assert got.dtype == np.int32 and np.array_equal(got, delays) and delays.any(), name
    assert same_state(final_state(s), want), name


def test_three_sessions_interleaved_equal_their_solo_runs(pipe, gpu, sources, solo, tmp_path):
    names = ("grid", "short48", "call")
    pipe.rttm_out_dir = str(tmp_path)
    try:
        hub = pipe.open_hub(max_sessions=4, max_seconds=60.0, array_channels=4, array_rate=48000)
        sessions = {name: hub.open(name, delta_new=DELTA, feed_format=sources[name][0]) for name in names}
        assert type(sessions["grid"]).__name__ == "LiveDiarization"
        assert sessions["grid"].ingest.array and sessions["short48"].ingest.array and not sessions["call"].ingest.array
        ticks = []

        def after_tick(out):
            t = dict(hub.stats["tick"])
            ticks.append(t)
            assert t["array_launches"] <= 1                                            # one wave per tick: ONE launch set
            assert t["array_calls"] <= 2 and (t["array_launches"] == 1) == (t["array_calls"] > 0)
            assert t["forwards"] == -(-t["windows"] // pipe._runner.batch_size)

        results = drive(hub, sessions, sources, after_tick)
        torch.cuda.synchronize()
        assert not hub.sessions and hub.stats["ticks"] == len(results)
        assert any(t["array_calls"] >= 2 and t["array_launches"] == 1 for t in ticks)
        tot = hub.stats["total"]
        assert tot == {k: sum(t[k] for t in ticks) for k in tot}
        assert hub.tick() == {} and hub.stats["tick"] == dict.fromkeys(hub.stats["tick"], 0)      # a tick without array work
        assert "array_calls" in hub.stats["tick"] and "array_launches" in hub.stats["tick"]
        assert tot["array_calls"] == sessions["grid"].ingest.uploads + sessions["short48"].ingest.uploads > tot["array_launches"]
        for name, s in sessions.items():
            check_against_solo(s, solo[name], name)
            assert name in [k for r in results for k in r]
            assert (tmp_path / f"{name}.rttm").read_text() == solo[name][4] == s.result.to_rttm()
        with pytest.raises(ValueError, match="not an array feed"):
            sessions["call"].ingest.delays()
        hub.close()
    finally:
        pipe.rttm_out_dir = None


def test_one_tick_after_several_feeds_takes_several_waves(pipe, gpu, sources, solo):
    with pipe.open_hub(max_sessions=2, max_seconds=60.0, array_channels=4) as hub:
        sessions = {"short16": hub.open("short16", delta_new=DELTA, feed_format=sources["short16"][0])}
        ticks = []
        drive(hub, sessions, sources, lambda out: ticks.append(dict(hub.stats["tick"])), per_round=3)
        torch.cuda.synchronize()
        assert max(t["array_launches"] for t in ticks) >= 3                            # three blocks' worth before one tick
        assert all(t["array_launches"] == t["array_calls"] for t in ticks)             # two calls of one session never share a wave
        check_against_solo(sessions["short16"], solo["short16"], "short16")


def test_a_reused_row_starts_from_a_zeroed_tracker(pipe, gpu, sources, solo):
    """max_sessions = 1: the 48 kHz array ends, the 16 kHz array opens in the same row and equals its solo run — the tracker
    state and the delay table of the row were zeroed"""
    with pipe.open_hub(max_sessions=1, max_seconds=60.0, array_channels=4, array_rate=48000) as hub:
        first = {"short48": hub.open("short48", delta_new=DELTA, feed_format=sources["short48"][0])}
        drive(hub, first, sources)
        check_against_solo(first["short48"], solo["short48"], "short48")
        torch.cuda.synchronize()
        assert hub.arrays["state"].any() and hub.arrays["delay"].any()                 # what the first session left behind
        second = {"short16": hub.open("short16", delta_new=DELTA, feed_format=sources["short16"][0])}
        assert second["short16"].ingest.row == first["short48"].ingest.row == 0
        hub.copy_stream.synchronize()
        assert not hub.arrays["state"].any() and not hub.arrays["delay"].any() and bool((hub.pool[0] == 0).all())
        drive(hub, second, sources)
        torch.cuda.synchronize()
        check_against_solo(second["short16"], solo["short16"], "short16")


def test_detection_hub_takes_an_array_feed(pipe, gpu, sources, tmp_path):
    from diarizen_amd.detection import VoiceActivityDetection
    det = VoiceActivityDetection(pipe)
    fmt, chunks = sources["short16"]
    s = run_solo(lambda f: det.open_stream(uri="short16", max_seconds=60.0, feed_format=f), fmt, chunks)
    want = (s.committed_activity, s.result.to_rttm(), s.ingest.dev_wave[:s.n].clone(), s.ingest.delays())
    with det.open_hub(max_sessions=2, max_seconds=60.0, array_channels=4) as hub:
        sessions = {"short16": hub.open("short16", feed_format=fmt)}
        assert type(sessions["short16"]).__name__ == "DetectionStream"
        drive(hub, sessions, sources)
        torch.cuda.synchronize()
        h = sessions["short16"]
        assert np.array_equal(h.committed_activity, want[0]) and h.result.to_rttm() == want[1]
        assert torch.equal(h.ingest.dev_wave[:h.n], want[2]) and np.array_equal(h.ingest.delays(), want[3])
        assert hub.stats["total"]["array_calls"] > 0


def test_the_default_hub_still_refuses_an_array_feed(pipe, gpu, sources):
    with pipe.open_hub(max_sessions=1, max_seconds=10.0) as hub:
        assert hub.arrays is None and hub.book.array_channels == 0
        with pytest.raises(ValueError, match="is an array feed .channel=Beamform.: a hub's rows share one batched ingest launch, "
                                             "which does not beamform; open the session on its own"):
            hub.open("room", feed_format=sources["grid"][0])
        assert hub.book.free == [0]                                                    # the refusal took no row
    with pytest.raises(ValueError, match="array_rate needs array_channels"):
        pipe.open_hub(max_sessions=1, max_seconds=10.0, array_rate=48000)
    with pipe.open_hub(max_sessions=1, max_seconds=10.0, array_channels=2) as hub:
        with pytest.raises(ValueError, match="array_channels = 2"):
            hub.open("room", feed_format=sources["grid"][0])
        assert hub.book.free == [0]
