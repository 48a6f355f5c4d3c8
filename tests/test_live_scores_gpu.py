"""Live per-speaker activity scores on the MI355X.  Kernel level: dzn_diarize_range_scores (csrc/post.hip) writes the bytes of
dzn_diarize_range and, as scores, the bits of dzn_speaker_scores and of postprocess.speaker_scores_range — on the
reference-made golden cases (tests/golden/scores_ref.npz) as one range and over partitions, and on synthetic arrays at every
lane layout's edges; refusals touch nothing.  Sessions: open_live(scores=True) against a replay (offline device stage with
scores -> online.OnlineSpeakers -> one dzn_speaker_scores call with K = 20), in a hub beside sessions without scores, after
finish(recluster=True); pipeline.stream / diarize_many with return_scores=True against __call__.  Every comparison is by bits."""
import copy
import ctypes as C

import numpy as np
import pytest

from _live_scores_cases import AGG, bits, bounds, case, partitions
from _stream_cases import FEED, RECORDINGS, feeds, samples

pytestmark = pytest.mark.gpu

FEED_LONG = 46400                                   # 2.9 s per feed (FEED: 0.37 s)
WINDOWS = {"grid": 11, "padded": 29, "short": 1}
DELTA = 0.2
KW = dict(delta_new=DELTA, max_seconds=60.0, slot_seconds=2.5, slots=3)


# ----------------------------------------------------------------------------- kernel level
def device(gpu, soft, hard, starts, duration, warm_up=(0.0, 0.0), seg=None):
    import torch
    from diarizen_amd.postprocess import aggregation_windows
    ham, wu = aggregation_windows(soft.shape[1], duration, warm_up)
    seg = np.zeros(soft.shape, np.uint8) if seg is None else seg
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)         # noqa: E731
    return dict(seg=t(seg), hard=t(hard.astype(np.int8)), soft=t(soft), start=t(starts.astype(np.int32)), ham=t(ham), wu=t(wu),
                C=soft.shape[0])


def fused(d, t0, t1, K, max_count=None, num_windows=None):
    """one dzn_diarize_range_scores call -> (count, active, activations, scores) on the host"""
    from diarizen_amd.postprocess import diarize_range_scores_launch
    out = diarize_range_scores_launch(d["seg"], d["hard"], d["soft"], d["C"] if num_windows is None else num_windows, d["start"],
                                      d["ham"], d["wu"], t0, t1, K, K if max_count is None else max_count, want_activations=True)
    return tuple(x.cpu().numpy() for x in out)


def plain(d, t0, t1, K, max_count=None):
    from diarizen_amd.postprocess import diarize_range_launch
    out = diarize_range_launch(d["seg"], d["hard"], d["C"], d["start"], t0, t1, K, K if max_count is None else max_count,
                               want_activations=True)
    return tuple(x.cpu().numpy() for x in out)


def whole_scores(d, T, K):
    """dzn_speaker_scores over [0, T) with K columns"""
    import torch
    from diarizen_amd.postprocess import _call
    _, L, S = d["soft"].shape
    out = torch.empty((T, K), device=d["soft"].device, dtype=torch.float32)
    _call("dzn_speaker_scores", d["soft"], d["hard"], d["C"], L, S, d["start"], d["ham"], d["wu"], T, K, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", AGG)
def test_scores_equal_the_reference_run_as_one_range_and_over_partitions(built_lib, gpu, name):
    from diarizen_amd.postprocess import speaker_scores_range
    c = case(name)
    d = device(gpu, c["soft"], c["hard"], c["starts"], c["duration"], c["warm_up"])
    T, K = c["T"], c["K"]
    assert np.array_equal(bits(whole_scores(d, T, K)), bits(c["ref"]))
    for what, cuts in partitions(c).items():
        parts = [fused(d, a, b, K) for a, b in bounds(T, cuts)]
        for (a, b), p in zip(bounds(T, cuts), parts):
            assert p[3].dtype == np.float32 and p[3].shape == (b - a, K) and p[0].shape == (b - a,)
        got = np.concatenate([p[3] for p in parts])
        assert np.array_equal(bits(got), bits(c["ref"])), (name, what)
    # every frame the windows cover and three beyond, 20 (or 32) columns: the restatement, the extra columns zero
    Kw, full = (20 if K <= 20 else 32), c["full"] + 3
    got = fused(d, 0, full, Kw)[3]
    want = speaker_scores_range(c["soft"], c["hard"], c["starts"], 0, full, Kw, c["duration"], warm_up=c["warm_up"])
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got[:T, :K]), bits(c["ref"]))
    assert not got[:, K:].any() and not got[c["full"]:].any()


def synthetic(K, Cn, seed):
    """random decisions, labels and soft scores on windows of L = 50 frames whose starts leave gaps: labels -2 and >= K, two
    local speakers of a window under one label, a NaN, frames no window covers"""
    g = np.random.default_rng(seed)
    L, S = 50, 4
    steps = g.integers(0, 40, size=Cn)
    steps[0] = 0
    if Cn > 1:
        steps[1] = 13                                                   # window 1 starts before frame 31 and covers it
    if Cn > 4:
        steps[Cn // 2] = L + 9                                          # a gap: 9 frames no window covers
    starts = np.cumsum(steps).astype(np.int32)
    seg = (g.random((Cn, L, S)) < 0.4).astype(np.uint8)
    soft = g.random((Cn, L, S), dtype=np.float32)
    hard = g.integers(-2, K + 1, size=(Cn, S)).astype(np.int8)          # -2, -1 (skipped), 0 .. K - 1, K (out of range)
    hard[0] = [0, 0, -2, K]                                             # two local speakers in label 0
    soft[0, 7, 1] = np.nan
    soft[Cn - 1, 0, 0] = np.nan
    return seg, soft, hard, starts, L


SHAPES = [(1, 255), (1, 256), (1, 257), (3, 63), (3, 64), (3, 65), (20, 7), (20, 8), (20, 9), (32, 7), (32, 8), (32, 9), (32, 1)]


@pytest.mark.parametrize("K,n", SHAPES)
def test_every_output_at_the_lane_layouts_edges(built_lib, gpu, K, n):
    """n = t1 - t0 frames around the 256 >> kp_log2 frames of a workgroup; t0 = 31 lies inside the first windows"""
    from diarizen_amd.postprocess import speaker_scores_range
    seg, soft, hard, starts, L = synthetic(K, 12, 100 * K + n)
    d = device(gpu, soft, hard, starts, 2.0, seg=seg)
    t0 = 31 if n < 200 else 0
    t1 = t0 + n
    T = int(starts[-1]) + L
    assert t0 == 0 or 0 < starts[1] < t0 < L                            # windows that start before t0 cover it
    got = fused(d, t0, t1, K, max_count=3)
    for a, b in zip(got[:3], plain(d, t0, t1, K, max_count=3)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    want = speaker_scores_range(soft, hard, starts, t0, t1, K, 2.0)
    assert got[3].shape == (n, K) and np.array_equal(bits(got[3]), bits(want))
    assert np.array_equal(bits(got[3]), bits(whole_scores(d, max(t1, 1), K)[t0:t1]))
    assert np.isfinite(got[3]).all()
    if n >= 200:                                                        # the whole recording: the gap and the NaN are inside
        gap = [t for t in range(T) if not ((starts <= t) & (t < starts + L)).any()]
        assert len(gap) >= 9 and max(gap) < n and not got[3][gap].any() and not got[0][gap].any()
        assert (got[3] > 0).any(axis=0).all()


def test_one_window_and_a_range_past_its_end(built_lib, gpu):
    from diarizen_amd.postprocess import speaker_scores_range
    seg, soft, hard, starts, L = synthetic(3, 1, 5)
    d = device(gpu, soft, hard, starts, 2.0, seg=seg)
    assert d["C"] == 1
    for t0, t1 in ((0, L), (0, L + 20), (L - 1, L + 1), (L, L + 5), (7, 8)):
        got = fused(d, t0, t1, 3)
        for a, b in zip(got[:3], plain(d, t0, t1, 3)):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(bits(got[3]), bits(speaker_scores_range(soft, hard, starts, t0, t1, 3, 2.0)))
    assert not fused(d, L, L + 5, 3)[3].any()
    # no window at all
    got = fused(d, 0, 9, 3, num_windows=0)
    assert not got[3].any() and not got[0].any()


def test_refusals_touch_nothing_and_nothing_is_written_past_the_range(built_lib, gpu):
    import torch
    lib = built_lib
    seg, soft, hard, starts, L = synthetic(4, 12, 11)
    d = device(gpu, soft, hard, starts, 2.0, seg=seg)
    cnt = torch.full((40,), 9, dtype=torch.uint8, device=gpu)
    active = torch.full((40, 32), 9, dtype=torch.uint8, device=gpu)
    act = torch.full((40, 32), -7, dtype=torch.int32, device=gpu)
    sc = torch.full((40, 32), -3.0, dtype=torch.float32, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(t0, t1, K=4, S=4, Cn=12, Ln=L, max_count=20, null=()):
        a = {k: (None if k in null else p(v)) for k, v in dict(seg=d["seg"], hard=d["hard"], soft=d["soft"], start=d["start"],
                                                               ham=d["ham"], wu=d["wu"], cnt=cnt, active=active, act=act,
                                                               sc=sc).items()}
        return lib.dzn_diarize_range_scores(a["seg"], a["hard"], a["soft"], Cn, Ln, S, a["start"], a["ham"], a["wu"], t0, t1, K,
                                            max_count, a["cnt"], a["active"], a["act"], a["sc"], st)

    def untouched():
        torch.cuda.synchronize()
        return (int(cnt.min()) == 9 == int(cnt.max()) and int(active.min()) == 9 == int(active.max())
                and int(act.min()) == -7 == int(act.max()) and float(sc.min()) == -3.0 == float(sc.max()))
    for args, kw in (((-1, 5), {}), ((10, 9), {}), ((0, 10), dict(K=0)), ((0, 10), dict(K=33)), ((0, 10), dict(S=9)),
                     ((0, 10), dict(S=0)), ((0, 10), dict(Ln=0)), ((0, 10), dict(Cn=-1)), ((0, 10), dict(max_count=-1)),
                     *(((0, 10), dict(null=(k,))) for k in ("seg", "hard", "soft", "start", "ham", "wu", "cnt", "active", "sc"))):
        assert call(*args, **kw) == -1, (args, kw)
    assert untouched()
    assert call(12, 12) == 0 and call(0, 0, null=("act",)) == 0          # empty: DZN_OK, no launch
    assert untouched()
    assert call(5, 15, null=("act",)) == 0                               # the activations are optional
    torch.cuda.synchronize()
    want = fused(d, 5, 15, 4, max_count=20)
    assert np.array_equal(cnt[:10].cpu().numpy(), want[0]) and int(cnt[10:].min()) == 9
    flat = active.reshape(-1).cpu().numpy()
    assert np.array_equal(flat[:40].reshape(10, 4), want[1]) and int(flat[40:].min()) == 9
    assert int(act.min()) == -7 == int(act.max())
    flat = sc.reshape(-1).cpu().numpy()
    assert np.array_equal(bits(flat[:40].reshape(10, 4)), bits(want[3])) and float(flat[40:].max()) == -3.0 == float(flat[40:].min())


# ----------------------------------------------------------------------------- sessions
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


_REPLAY, _SOLO = {}, {}


def replay(pipe, gpu, name):
    """per recording, once: (samples, WAV bytes, scores f32 [T, 20]) — the offline device stage with scores, OnlineSpeakers
    over its windows in order, ONE dzn_speaker_scores call with K = 20 over every frame the windows cover"""
    if name not in _REPLAY:
        import torch
        from diarizen_amd.online import OnlineSpeakers
        from diarizen_amd.postprocess import _frame_grid, receptive_field
        x, data = samples(RECORDINGS[name])
        seg, emb, soft = pipe.device_stage(x, with_scores=True)
        Cn, L, S = seg.shape
        assert Cn == WINDOWS[name] and tuple(soft.shape) == (Cn, L, S) and soft.is_cuda
        K = min(pipe.max_speakers, 32)
        assert K == 20
        o = OnlineSpeakers(DELTA, K, emb.shape[2])
        hard = np.stack([o.assign(seg[c], emb[c]) for c in range(Cn)])
        _, starts, T = _frame_grid(Cn, L, pipe.chunks_window(), receptive_field())
        d = device(gpu, soft.cpu().numpy(), hard, starts, pipe.chunks_window().duration)
        sc = whole_scores(d, T, K)
        sc.setflags(write=False)
        _REPLAY[name] = (x, data, sc)
    return _REPLAY[name]


def final_state(sess, ann):
    return (sess.committed_diarization, sess.committed_count, sess.hard_clusters, ann.to_rttm(), sess.stats["range_calls"],
            sess.committed_scores)


def solo(pipe, gpu, name, scores, size=FEED_LONG):
    """a solo session fed in `size` chunks to the end, once per (name, scores, size): its final state"""
    key = (name, scores, size)
    if key not in _SOLO:
        x = replay(pipe, gpu, name)[0]
        sess = pipe.open_live(sess_name=name, scores=scores, **KW)
        for c in feeds(x, size):
            sess.feed(c)
        _SOLO[key] = final_state(sess, sess.finish())
    return _SOLO[key]


@pytest.mark.parametrize("name,size", [("grid", FEED), ("padded", FEED), ("short", FEED), ("padded", FEED_LONG)])
def test_committed_scores_only_grow_and_equal_the_replay(pipe, gpu, name, size):
    from diarizen_amd.core import SlidingWindowFeature
    x, _, ref = replay(pipe, gpu, name)
    K = ref.shape[1]
    sess = pipe.open_live(sess_name=name, scores=True, **KW)
    assert tuple(sess.soft.shape) == tuple(sess.seg.shape) and sess.soft.dtype.is_floating_point and sess.final_scores is None
    prev, grew = np.zeros((0, K), np.float32), 0
    for c in feeds(x, size):
        sess.feed(c)
        sc = sess.committed_scores
        F = len(sc)
        assert sc.dtype == np.float32 and sc.shape == (F, K) and F == len(sess.committed_diarization) >= len(prev)
        assert np.array_equal(bits(sc[:len(prev)]), bits(prev)) and np.array_equal(bits(sc), bits(ref[:F]))
        grew += F > len(prev)
        live = sess.scores
        assert isinstance(live, SlidingWindowFeature) and live.data.shape == (sess.covered, K) and live.sliding_window is sess.grid
        assert np.array_equal(bits(live.data[:F]), bits(sc))
        prev = sc
    assert (grew == 0 and len(prev) == 0) if name == "short" else (grew >= 5 and 0 < len(prev) < len(ref))
    ann = sess.finish()
    assert np.array_equal(bits(sess.committed_scores), bits(ref)) and np.array_equal(bits(sess.final_scores), bits(ref))
    assert len(sess.committed_scores) == len(sess.committed_diarization) == len(ref)
    assert np.isfinite(ref).all() and (name == "short" or (ref > 0).any())
    _SOLO.setdefault((name, True, size), final_state(sess, ann))


@pytest.mark.parametrize("name", list(RECORDINGS))
def test_everything_else_is_what_a_session_without_scores_gives(pipe, gpu, name):
    with_, without = solo(pipe, gpu, name, True), solo(pipe, gpu, name, False)
    for a, b in zip(with_[:5], without[:5]):                            # diarization, count, labels, RTTM text, range calls
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert without[5] is None and with_[4] >= 1
    sess = pipe.open_live(sess_name=name, **KW)
    assert sess.soft is None and sess.scores is None and sess.committed_scores is None and "score" not in sess.rows._rows


def test_stream_live_yields_the_scores(pipe, gpu):
    x, _, ref = replay(pipe, gpu, "grid")
    out = list(pipe.stream_live(feeds(x, FEED_LONG), sess_name="grid", scores=True, **KW))
    assert all(len(item) == 4 for item in out) and len(out) >= 2
    for secs, committed, ann, sc in out[:-1]:
        F = round(committed / 0.02)
        assert np.array_equal(bits(sc.data[:F]), bits(ref[:F])) and len(sc.data) > F
    assert np.array_equal(bits(out[-1][3].data), bits(ref))
    assert all(len(item) == 3 for item in pipe.stream_live(feeds(x[:140000], FEED_LONG), sess_name="grid", **KW))


def test_recluster_gives_the_offline_scores_under_the_live_labels(pipe, gpu):
    x, data, ref = replay(pipe, gpu, "padded")
    ann_off, off = pipe(data, sess_name="padded", return_scores=True)
    sess = pipe.open_live(sess_name="padded", scores=True, **KW)
    for c in feeds(x, FEED_LONG):
        sess.feed(c)
    ann = sess.finish(recluster=True)
    m, fs = sess.label_map, sess.final_scores
    Ko = off.data.shape[1]
    assert set(range(Ko)) <= set(m) and Ko >= 2                          # (the discrete diarization may have padded columns)
    assert fs.dtype == np.float32 and fs.shape == (len(off.data), max(20, max(m.values()) + 1)) and len(fs) < len(ref)
    for i in range(Ko):
        assert np.array_equal(bits(fs[:, m[i]]), bits(off.data[:, i]))
    assert not fs[:, sorted(set(range(fs.shape[1])) - {m[i] for i in range(Ko)})].any()
    assert np.array_equal(bits(sess.committed_scores), bits(ref))       # the committed arrays stay the live ones
    back = {v: k for k, v in m.items()}
    turns = lambda a, f: sorted((s.start, s.end, f(lab)) for s, _, lab in a.itertracks(yield_label=True))      # noqa: E731
    assert turns(ann, lambda lab: back[lab]) == turns(ann_off, lambda lab: lab)


def run_hub(pipe, gpu, want):
    """grid, padded and short in one hub, fed round-robin in 2.9 s chunks with a tick per round -> ({name: final state},
    the hub's totals)"""
    xs = {name: replay(pipe, gpu, name)[0] for name in want}
    with pipe.open_hub(max_sessions=4, max_seconds=60.0) as hub:
        sessions = {name: hub.open(name, delta_new=DELTA, scores=sc) for name, sc in want.items()}
        todo = {name: feeds(xs[name], FEED_LONG) for name in want}
        open_ = set(want)
        while open_:
            for name in sorted(open_):
                if todo[name]:
                    sessions[name].feed(todo[name].pop(0))
                else:
                    assert sessions[name].finish() is None
                    open_.discard(name)
            hub.tick()
        return {name: final_state(s, s.result) for name, s in sessions.items()}, dict(hub.stats["total"])


def test_hub_sessions_have_the_bits_of_their_solo_runs(pipe, gpu):
    want = {"grid": True, "padded": False, "short": True}
    got, total = run_hub(pipe, gpu, want)
    for name, sc in want.items():
        ref = solo(pipe, gpu, name, sc)
        for i, (a, b) in enumerate(zip(got[name], ref)):
            if i == 4:                                                   # range calls: the hub's ticks are its own chunking
                continue
            if a is None or b is None:
                assert a is None and b is None and not sc
            else:
                assert (np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)) \
                    if isinstance(a, np.ndarray) else a == b, (name, i)
    assert np.array_equal(bits(got["grid"][5]), bits(replay(pipe, gpu, "grid")[2]))
    assert np.array_equal(bits(got["short"][5]), bits(replay(pipe, gpu, "short")[2]))
    none, total0 = run_hub(pipe, gpu, dict.fromkeys(want, False))
    assert total["forwards"] == total0["forwards"] > 0 and total == total0
    for name in want:
        for a, b in zip(got[name][:5], none[name][:5]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_stream_return_scores_final_equals_call(pipe, gpu):
    x, data, _ = replay(pipe, gpu, "padded")
    ann_off, off = pipe(data, sess_name="padded", return_scores=True)
    out = list(pipe.stream(feeds(x, FEED_LONG), sess_name="padded", return_scores=True, refresh_s=8.0, **{
        k: v for k, v in KW.items() if k != "delta_new"}))
    assert len(out) >= 3 and all(len(item) == 3 for item in out)
    secs, ann, sc = out[-1]
    assert secs == len(x) / 16000 and ann.to_rttm() == ann_off.to_rttm()
    assert sc.data.shape == off.data.shape and np.array_equal(bits(sc.data), bits(off.data))
    assert sc.sliding_window.step == off.sliding_window.step and sc.sliding_window.start == off.sliding_window.start
    for _, a, s in out[:-1]:                                             # a refresh: the scores of the windows so far, no crop
        assert s.data.dtype == np.float32 and s.data.ndim == 2 and 0 < len(s.data) < len(off.data) + 100
    plain_out = list(pipe.stream(feeds(x[:140000], FEED_LONG), sess_name="grid"))
    assert all(len(item) == 2 for item in plain_out)


def test_diarize_many_return_scores_equals_two_calls(pipe, gpu, monkeypatch):
    datas = [replay(pipe, gpu, name)[1] for name in ("grid", "padded")]
    want = [pipe(d, sess_name=n, return_scores=True) for d, n in zip(datas, ("grid", "padded"))]
    for overlap in (True, False):
        got = list(pipe.diarize_many(datas, sess_names=["grid", "padded"], overlap=overlap, return_scores=True))
        assert [g[0] for g in got] == ["grid", "padded"] and all(len(g) == 3 for g in got)
        for (_, ann, sc), (ann0, sc0) in zip(got, want):
            assert ann.to_rttm() == ann0.to_rttm()
            assert sc.data.shape == sc0.data.shape and np.array_equal(bits(sc.data), bits(sc0.data))
    assert all(len(g) == 2 for g in pipe.diarize_many(datas[:1], sess_names=["grid"]))
    monkeypatch.setattr("diarizen_amd.dist.world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="runs on one device"):
        next(pipe.diarize_many(datas, sess_names=["grid", "padded"], return_scores=True))
