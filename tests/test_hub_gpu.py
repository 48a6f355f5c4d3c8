"""A live hub (diarizen_amd/hub.py, pipeline.open_hub) on the MI355X: three diarization sessions — float32 feeds, a 48 kHz int16
microphone, an 8 kHz two-channel mu-law call in packets that end inside a frame — fed interleaved in unequal chunking with one
tick() per round.  Every session must end with the committed arrays, labels, RTTM and waveform of the same feeds through
pipeline.open_live ALONE, bit for bit, while the hub runs one upload, at most one ingest launch and ceil(windows / batch_size)
forwards per tick; then finish(recluster=True), the reuse of a finished session's row, and the detection hubs."""
from __future__ import annotations

import audioop
import copy
import os

import numpy as np
import pytest
import torch

from _stream_cases import FEED, RECORDINGS, feeds, samples

pytestmark = pytest.mark.gpu

DELTA = 0.2                                         # the seeded embedding weights: 3 speakers at 0.2
PACKET = 5921                                       # bytes of the mu-law call per feed: ends inside a frame
MIC_CHUNK = 99999                                   # bytes of the 48 kHz int16 feed per feed: ends inside a sample


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    """the seeded wavlm_large_s80_md pipeline of tests/test_live_diarization_gpu.py: 8 s windows, batches of 64"""
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


@pytest.fixture(scope="module")
def sources():
    """name -> (feed_format or None, the chunks of its feed loop)"""
    from diarizen_amd.audio import FeedFormat, resample
    out = {"grid": (None, feeds(samples(RECORDINGS["grid"])[0], FEED))}
    x48 = resample(samples(RECORDINGS["padded"])[0], 16000, 48000)
    mic = np.clip(np.rint(x48 * 32768.0), -32768, 32767).astype("<i2").tobytes()
    out["padded"] = (FeedFormat(48000, "s16", channel=0), [mic[i:i + MIC_CHUNK] for i in range(0, len(mic), MIC_CHUNK)])
    # the call of tests/test_feed_sessions_gpu.py: 8 kHz, two channels (channel 1 = channel 0 delayed by 0.5 s), mu-law
    x8 = resample(samples(RECORDINGS["short"])[0], 16000, 8000)
    x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)
    body = audioop.lin2ulaw(np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes(), 2)
    assert len(body) == 80000 and len(body) % PACKET and PACKET % 2 and len(mic) % MIC_CHUNK and MIC_CHUNK % 2
    out["short"] = (FeedFormat(8000, "ulaw", channels=2, channel=1), [body[i:i + PACKET] for i in range(0, len(body), PACKET)])
    assert len({len(chunks) for _, chunks in out.values()}) == 3                     # unequal chunking: 44 / 29 / 14 feeds
    return out


def final_state(sess):
    return (sess.committed_diarization, sess.committed_count, sess.hard_clusters, sess.result.to_rttm())


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def run_solo(open_session, fmt, chunks, **finish_kw):
    sess = open_session(fmt)
    for c in chunks:
        sess.feed(c)
    sess.finish(**finish_kw)
    torch.cuda.synchronize()
    return sess


@pytest.fixture(scope="module")
def solo(pipe, sources, tmp_path_factory):
    """name -> (final state, dev_wave[:n], n, RTTM file's text) of the session ALONE (pipeline.open_live)"""
    d = tmp_path_factory.mktemp("solo")
    pipe.rttm_out_dir = str(d)
    out = {}
    try:
        for name, (fmt, chunks) in sources.items():
            s = run_solo(lambda f: pipe.open_live(sess_name=name, delta_new=DELTA, max_seconds=60.0, feed_format=f), fmt, chunks)
            out[name] = (final_state(s), s.ingest.dev_wave[:s.n].clone(), s.n, (d / f"{name}.rttm").read_text())
            del s
    finally:
        pipe.rttm_out_dir = None
    return out


def drive(hub, sessions, sources, after_tick=None, finish_kw=None):
    """feed round-robin, one chunk per session and round, finish() a session once its chunks are out, tick() after every
    round; -> the ticks' results"""
    todo = {name: list(sources[name][1]) for name in sessions}
    open_ = set(sessions)
    results = []
    while open_:
        for name in sorted(open_):
            if todo[name]:
                assert sessions[name].feed(todo[name].pop(0)) is sessions[name]._last      # host only: nothing new before the tick
            else:
                assert sessions[name].finish(**(finish_kw or {})) is None
                open_.discard(name)
        out = hub.tick()
        results.append(out)
        if after_tick is not None:
            after_tick(out)
    return results


def test_three_sessions_interleaved_equal_their_solo_runs(pipe, gpu, sources, solo, tmp_path):
    from diarizen_amd.postprocess import committed_frames
    pipe.rttm_out_dir = str(tmp_path)
    try:
        hub = pipe.open_hub(max_sessions=4, max_seconds=60.0)
        sessions = {name: hub.open(name, delta_new=DELTA, feed_format=sources[name][0]) for name in sources}
        assert type(sessions["grid"]).__name__ == "LiveDiarization" and hub.pool.shape == (4, 60 * 16000 + 128000)
        snaps = {name: [] for name in sessions}
        ticks = []

        def after_tick(out):
            t = dict(hub.stats["tick"])
            ticks.append(t)
            assert t["ingest_launches"] <= t["uploads"] <= 1                          # every round fits one slot
            assert t["forwards"] == -(-t["windows"] // pipe._runner.batch_size)
            assert t["sessions_advanced"] == len(out)
            for name, s in sessions.items():
                assert s.frontier == committed_frames(s.done, s.chunks, s.frames, s.grid) or s.result is not None
                assert s.done == len(s.hard_clusters) == s.stats["windows"]
                snaps[name].append((s.committed_diarization, s.committed_count, s.hard_clusters))
                if name in out:
                    assert out[name] is s._last and out[name].uri == name

        results = drive(hub, sessions, sources, after_tick)
        torch.cuda.synchronize()
        assert not hub.sessions and hub.stats["ticks"] == len(results) == 45          # 44 feeds of the longest + its finish
        assert any(t["forwards"] < t["sessions_advanced"] for t in ticks)             # windows of several sessions in ONE forward
        assert any(t["uploads"] == 1 and t["ingest_launches"] == 1 for t in ticks)
        tot = hub.stats["total"]
        assert tot == {k: sum(t[k] for t in ticks) for k in tot} and tot["windows"] == 11 + 29 + 1
        assert tot["range_calls"] == sum(s.stats["range_calls"] for s in sessions.values()) > 0
        assert tot["forwards"] < tot["sessions_advanced"]
        for name, s in sessions.items():
            want, wave, n, rttm = solo[name]
            assert s.finished and s.n == n and name in [k for r in results for k in r]
            assert torch.equal(s.ingest.dev_wave[:n], wave), name                      # the pool row is the solo waveform
            assert bool((s.ingest.dev_wave[n:] == 0).all())
            assert same_state(final_state(s), want), name
            assert (tmp_path / f"{name}.rttm").read_text() == rttm == s.result.to_rttm()
            final = final_state(s)
            for a, c, h in snaps[name]:                                               # after every tick: a prefix of the final arrays
                assert np.array_equal(a, final[0][:len(a)]) and np.array_equal(c, final[1][:len(c)])
                assert np.array_equal(h, final[2][:len(h)])
            assert [len(a) for a, _, _ in snaps[name]] == sorted(len(a) for a, _, _ in snaps[name])
        with pytest.raises(RuntimeError, match="already finished"):
            sessions["grid"].feed(np.zeros(16, dtype=np.float32))
        hub.close()
        with pytest.raises(RuntimeError, match="closed"):
            hub.tick()
    finally:
        pipe.rttm_out_dir = None


def test_refusals_on_an_open_hub(pipe, gpu):
    from diarizen_amd.audio import FeedFormat
    with pipe.open_hub(max_sessions=2, max_seconds=10.0) as hub:
        a = hub.open("a")
        with pytest.raises(ValueError, match="already open"):
            hub.open("a")
        with pytest.raises(ValueError, match="does not fit in LDS"):
            hub.open("b", feed_format=FeedFormat(15999, "s16", channel=0))
        with pytest.raises(ValueError, match="FeedFormat"):
            hub.open("b", feed_format="ulaw")
        with pytest.raises(ValueError, match="channel"):
            hub.open("b", feed_format=FeedFormat(8000, "ulaw", channel=1))              # channel 1 of a mono feed
        with pytest.raises(TypeError, match="max_seconds"):
            hub.open("b", max_seconds=5.0)
        assert hub.book.free == [1]                                                    # the refusals took no row
        hub.open("b", feed_format=FeedFormat(8000, "ulaw", channels=2))                # the pipeline's channel
        with pytest.raises(RuntimeError, match="max_sessions = 2"):
            hub.open("c")
        a.feed(np.zeros(16000 * 9, dtype=np.float32))
        with pytest.raises(MemoryError, match="max_seconds = 10 s"):
            a.feed(np.zeros(16001, dtype=np.float32))
        out = hub.tick()                                                               # 9 s: two complete windows
        assert list(out) == ["a"] and a.n == 16000 * 9 and a.done == 2 and hub.stats["tick"]["uploads"] == 1
        assert hub.tick() == {} and hub.stats["tick"] == dict.fromkeys(hub.stats["tick"], 0)      # nothing fed: no device work
        a.finish()
        with pytest.raises(RuntimeError, match="already finished"):
            a.feed(np.zeros(1, dtype=np.float32))
        with pytest.raises(RuntimeError, match="already finished"):
            a.finish()
        out = hub.tick()
        assert list(out) == ["a"] and out["a"] is a.result and a.done == 3 and hub.book.free == [0]      # + the zero-padded window


def test_recluster_through_the_hub_equals_the_solo_result(pipe, gpu, sources):
    fmt, chunks = sources["grid"]
    s = run_solo(lambda f: pipe.open_live(sess_name="grid", delta_new=DELTA, max_seconds=60.0, feed_format=f), fmt, chunks,
                 recluster=True)
    with pipe.open_hub(max_sessions=2, max_seconds=60.0) as hub:
        sessions = {"grid": hub.open("grid", delta_new=DELTA)}
        results = drive(hub, sessions, sources, finish_kw={"recluster": True})
        h = sessions["grid"]
        assert results[-1]["grid"] is h.result
        assert same_state(final_state(h), final_state(s)) and h.label_map == s.label_map and h.label_map is not None
        assert h.num_speakers == s.num_speakers


def test_a_reused_row_reads_zeros_behind_the_new_session(pipe, gpu, sources, solo):
    """max_sessions = 1: `padded` (30 s) ends, `short` (5 s) opens in the same row; its zero-padded window reads the pool
    behind its 5 s — zeros, not the previous call's samples"""
    with pipe.open_hub(max_sessions=1, max_seconds=60.0) as hub:
        first = {"padded": hub.open("padded", delta_new=DELTA, feed_format=sources["padded"][0])}
        with pytest.raises(RuntimeError, match="max_sessions = 1"):
            hub.open("short", delta_new=DELTA, feed_format=sources["short"][0])
        drive(hub, first, sources)
        assert same_state(final_state(first["padded"]), solo["padded"][0])
        second = {"short": hub.open("short", delta_new=DELTA, feed_format=sources["short"][0])}
        assert second["short"].ingest.row == first["padded"].ingest.row == 0
        torch.cuda.synchronize()
        assert bool((hub.pool[0] == 0).all())
        drive(hub, second, sources)
        torch.cuda.synchronize()
        want, wave, n, _ = solo["short"]
        assert torch.equal(hub.pool[0, :n], wave) and bool((hub.pool[0, n:] == 0).all())
        assert same_state(final_state(second["short"]), want)


@pytest.mark.parametrize("kind", ["VoiceActivityDetection", "OverlappedSpeechDetection"])
def test_detection_hub_equals_the_solo_streams(pipe, gpu, sources, kind, tmp_path):
    from diarizen_amd import detection
    det = getattr(detection, kind)(pipe, rttm_out_dir=str(tmp_path / "solo"))
    os.makedirs(tmp_path / "hub")
    names = ("grid", "short")
    want = {}
    for name in names:
        fmt, chunks = sources[name]
        s = run_solo(lambda f: det.open_stream(uri=name, max_seconds=60.0, feed_format=f), fmt, chunks)
        want[name] = (s.committed_activity, s.result.to_rttm())
    det.rttm_out_dir = str(tmp_path / "hub")
    with det.open_hub(max_sessions=2, max_seconds=60.0) as hub:
        sessions = {name: hub.open(name, feed_format=sources[name][0]) for name in names}
        assert type(sessions["grid"]).__name__ == "DetectionStream"
        prefixes = {name: [] for name in names}
        drive(hub, sessions, sources, lambda out: [prefixes[n].append(sessions[n].committed_activity) for n in names])
        assert hub.stats["total"]["windows"] == 11 + 1 and hub.stats["total"]["forwards"] <= hub.stats["total"]["windows"]
        for name in names:
            s = sessions[name]
            assert np.array_equal(s.committed_activity, want[name][0]) and s.result.to_rttm() == want[name][1]
            assert all(np.array_equal(p, want[name][0][:len(p)]) for p in prefixes[name])
            assert (tmp_path / "hub" / f"{name}.rttm").read_text() == (tmp_path / "solo" / f"{name}.rttm").read_text()
