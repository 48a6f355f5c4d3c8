"""Live speaker diarization (diarizen_amd/live.py, LiveDiarization) on the MI355X: audio fed in 0.37 s chunks.  After every
feed each window was computed once and the committed diarization / count only grew; after finish() they and the labels equal
a replay (offline device stage -> online.OnlineSpeakers over its windows on the host -> one dzn_diarize_range call) bit for
bit, whatever the chunking; a label keeps its committed frames from one provisional annotation to the next; finish(
recluster=True) gives the offline turns under the live labels."""
import copy

import numpy as np
import pytest

from _stream_cases import FEED, RECORDINGS, STEP, WINDOW, feeds, samples

FEED_LONG = 46400                                   # 2.9 s per feed (FEED: 0.37 s)
WINDOWS = {"grid": 11, "padded": 29, "short": 1}
DELTA = 0.2                                         # the seeded embedding weights: 3 speakers at 0.2 (16 at the config's 0.1)
KW = dict(delta_new=DELTA, max_seconds=60.0, slot_seconds=2.5, slots=3)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
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


_REPLAY = {}


def replay(pipe, gpu, name):
    """per recording, once: (samples, WAV bytes, hard [C, S], count [T], diarization [T, K]) — the offline device stage of
    the whole recording, OnlineSpeakers over its windows in order, one dzn_diarize_range(0, T) call"""
    if name not in _REPLAY:
        import torch
        from diarizen_amd.online import OnlineSpeakers
        from diarizen_amd.postprocess import _frame_grid, diarize_range_launch, receptive_field
        x, data = samples(RECORDINGS[name])
        seg, emb = pipe.device_stage(x)
        Cn, L, S = seg.shape
        assert Cn == WINDOWS[name] and (L, S) == (399, 4)
        K = min(pipe.max_speakers, 32)
        o = OnlineSpeakers(DELTA, K, emb.shape[2])
        hard = np.stack([o.assign(seg[c], emb[c]) for c in range(Cn)])
        _, starts, T = _frame_grid(Cn, L, pipe.chunks_window(), receptive_field())
        cnt, act, _ = diarize_range_launch(torch.from_numpy(seg).to(gpu), torch.from_numpy(hard).to(gpu), Cn,
                                           torch.from_numpy(starts).to(gpu), 0, T, K, K)
        out = (x, data, hard, cnt.cpu().numpy(), act.cpu().numpy(), o.num_speakers)
        for a in out[2:5]:
            a.setflags(write=False)
        _REPLAY[name] = out
    return _REPLAY[name]


def raster(ann, n, K):
    """Annotation -> bool [n, K] per-frame activity of the integer labels (a region runs from the middle of the frame that
    switched on to the middle of the first frame that is off)"""
    ts = np.arange(n) * 0.02 + 0.0125
    out = np.zeros((n, K), dtype=bool)
    for seg, _, lab in ann.itertracks(yield_label=True):
        out[:, int(lab)] |= (ts >= seg.start - 1e-6) & (ts < seg.end - 1e-6)
    return out


def final_state(sess, ann):
    return (sess.committed_diarization, sess.committed_count, sess.hard_clusters, ann.to_rttm())


@pytest.mark.parametrize("name", list(RECORDINGS))
def test_committed_prefix_after_every_feed_and_replay_at_the_end(pipe, gpu, name):
    from diarizen_amd.streaming import complete_windows
    x, _, hard, cnt, act, nspk = replay(pipe, gpu, name)
    K = act.shape[1]
    assert K == 20
    sess = pipe.open_live(sess_name=name, **KW)
    prev_a, prev_c, prev_ann, seen = np.zeros((0, K), np.uint8), np.zeros(0, np.uint8), None, 0
    for c in feeds(x):
        ann = sess.feed(c)
        done = complete_windows(sess.n, WINDOW, STEP)
        assert sess.done == done == sess.stats["windows"] == len(sess.hard_clusters)      # each window once, when complete
        a, cc = sess.committed_diarization, sess.committed_count
        F = len(a)
        assert a.dtype == np.uint8 and cc.dtype == np.uint8 and a.shape == (F, K) and cc.shape == (F,)
        assert F >= len(prev_a) and np.array_equal(a[:len(prev_a)], prev_a) and np.array_equal(cc[:len(prev_c)], prev_c)
        assert F == (0 if done == 0 else round(done * STEP / 320))            # the start frame of the next window
        assert sess.committed_seconds == pytest.approx(F * 0.02) and sess.seconds == sess.n / 16000
        assert sess.committed_seconds <= sess.seconds
        assert np.array_equal(a, act[:F]) and np.array_equal(cc, cnt[:F]) and np.array_equal(sess.hard_clusters, hard[:done])
        if done == 0:
            assert ann is None
        else:
            assert ann is not None and ann.uri == name
            labels = {lab for _, _, lab in ann.itertracks(yield_label=True)}
            # integer labels as offline; a column beyond num_speakers can be active, as in the reference's selection: where the
            # count asks for more speakers than have an activation, zero activations are taken in ascending k
            assert all(isinstance(lab, (int, np.integer)) and 0 <= lab < K for lab in labels)
            r = raster(ann, F, K)
            assert np.array_equal(r, a.astype(bool))                          # the annotation shows the committed frames
            if prev_ann is not None:                                          # ... and a label keeps them from feed to feed
                assert np.array_equal(raster(prev_ann, len(prev_a), K), r[:len(prev_a)])
            seen += 1
            prev_ann = ann
        prev_a, prev_c = a, cc
    if name == "short":
        assert seen == 0 and len(prev_a) == 0
    else:
        assert seen > 10 and 0 < len(prev_a) < len(act)
    final = sess.finish()
    assert sess.stats["windows"] == sess.done == WINDOWS[name]
    assert sess.stats["range_calls"] <= sess.stats["launches"] + 1 and sess.stats["uploads"] >= len(feeds(x))
    assert np.array_equal(sess.committed_diarization, act) and np.array_equal(sess.committed_count, cnt)
    assert np.array_equal(sess.hard_clusters, hard) and sess.num_speakers == nspk
    assert np.array_equal(sess.committed_diarization[:len(prev_a)], prev_a)
    assert sess.committed_seconds == pytest.approx(len(act) * 0.02)
    assert np.array_equal(raster(final, len(act), K)[:-1], act.astype(bool)[:-1])
    if name == "padded":
        # the case is not degenerate: several speakers, not one per window, and overlapped speech in the committed frames
        print(f"{name}: {sess.num_speakers} speakers, {int((cnt == 2).sum())} of {len(cnt)} frames with count 2")
        assert 2 <= sess.num_speakers <= 8
        assert (cnt == 2).any()
    with pytest.raises(RuntimeError):
        sess.feed(x[:10])
    with pytest.raises(RuntimeError):
        sess.finish()


def test_chunking_changes_nothing(pipe, gpu):
    """0.37 s chunks and 2.9 s chunks (three or four windows per feed): identical arrays and RTTM text"""
    x, _, hard, cnt, act, _ = replay(pipe, gpu, "padded")
    got = []
    for size in (FEED, FEED_LONG):
        sess = pipe.open_live(sess_name="padded", **KW)
        for c in feeds(x, size):
            sess.feed(c)
        got.append(final_state(sess, sess.finish()))
        assert sess.stats["windows"] == 29
    assert sess.stats["launches"] < 15                                        # the long chunks batch their windows
    for a, b in zip(*got):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(got[0][0], act) and np.array_equal(got[0][2], hard)
    assert len(got[0][3].splitlines()) >= 2


def test_recluster_gives_the_offline_turns_under_live_labels(pipe, gpu):
    x, data, _, _, act, nspk = replay(pipe, gpu, "padded")
    offline = pipe(data, sess_name="padded")
    sess = pipe.open_live(sess_name="padded", **KW)
    for c in feeds(x, FEED_LONG):
        sess.feed(c)
    ann = sess.finish(recluster=True)
    m = sess.label_map
    offline_labels = {lab for _, _, lab in offline.itertracks(yield_label=True)}
    assert offline_labels <= set(m) and len(set(m.values())) == len(m)        # every offline cluster, injective
    back = {v: k for k, v in m.items()}
    turns = lambda a, f: sorted((s.start, s.end, f(lab)) for s, _, lab in a.itertracks(yield_label=True))      # noqa: E731
    assert turns(ann, lambda lab: back[lab]) == turns(offline, lambda lab: lab)
    assert len(turns(ann, int)) > 0
    # matched offline clusters carry a live label, the others fresh ones from num_speakers upward
    assert any(v < nspk for v in m.values()) and all(0 <= v < nspk + len(m) for v in m.values())
    assert np.array_equal(sess.committed_diarization, act)                    # the committed arrays stay the live ones


def test_generator_form_and_rttm_file(pipe, gpu, tmp_path):
    x, _, _, _, act, _ = replay(pipe, gpu, "grid")
    pipe.rttm_out_dir = str(tmp_path)
    try:
        out = list(pipe.stream_live(feeds(x), sess_name="grid", **KW))
    finally:
        pipe.rttm_out_dir = None
    secs, committed, ann = out[-1]
    assert secs == len(x) / 16000 and committed == pytest.approx(len(act) * 0.02)
    assert len(out) > 10 and all(c <= s for s, c, _ in out[:-1])
    assert [t[0] for t in out] == sorted(t[0] for t in out) and [t[1] for t in out] == sorted(t[1] for t in out)
    text = (tmp_path / "grid.rttm").read_text()
    assert text == ann.to_rttm() and text.startswith("SPEAKER grid ")
    assert np.array_equal(raster(ann, len(act), act.shape[1])[:-1], act.astype(bool)[:-1])
    # no session name: no file is asked for
    sess = pipe.open_live(**KW)
    assert sess.finish().uri is None and sess.seconds == 0.0


def test_refuses_distributed_runs(pipe, gpu, monkeypatch):
    monkeypatch.setattr("diarizen_amd.dist.world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="runs on one device"):
        pipe.open_live(sess_name="x")
