"""dzn_detect_range (csrc/post.hip) on the MI355X: the concatenation of range calls — scores and activity, the hysteresis
state carried from call to call — equals one dzn_detect call over all frames bit for bit, wherever the cuts fall; a range
without a decisive frame keeps its entry state; bad arguments are refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ONSET, OFFSET = 0.7, 0.3        # frames with offset <= y <= onset keep the state, so the carried state matters
TASKS = 3


def blocky(seed, Cn, L, S=4):
    """per (window, speaker) runs that toggle with probability 6 % per frame"""
    g = np.random.default_rng(seed)
    tog = g.random((Cn, L, S)) < 0.06
    tog[:, 0, :] = g.random((Cn, S)) < 0.4
    return (np.cumsum(tog, axis=1) % 2).astype(np.uint8)


def _chunks():
    from diarizen_amd.core import SlidingWindow
    return SlidingWindow(start=0.0, duration=2.0, step=0.1 * 2.0)


_REF = {}


def reference(gpu, Cn, L=99):
    """(device decisions, whole-recording scores [T, 2], activity [T, 2], window start frames): one dzn_detect call, shared"""
    if (Cn, L) not in _REF:
        import torch
        from diarizen_amd.postprocess import _frame_grid, detect_device, receptive_field
        seg = torch.from_numpy(blocky(100 + Cn, Cn, L)).to(gpu)
        act, sc, _ = detect_device(seg, _chunks(), receptive_field(), TASKS, onset=ONSET, offset=OFFSET, want_scores=True)
        _, starts, T = _frame_grid(Cn, L, _chunks(), receptive_field())
        assert act.shape == sc.shape == (T, 2)
        act.setflags(write=False)
        sc.setflags(write=False)
        _REF[(Cn, L)] = (seg, sc, act, starts, T)
    return _REF[(Cn, L)]


def run_ranges(seg, cuts, T):
    """range calls over [0, c1), [c1, c2), ... [cn, T): each starts from the last activity row of the one before"""
    from diarizen_amd.postprocess import detect_device, receptive_field
    bounds = [0] + [int(c) for c in cuts] + [T]
    assert bounds == sorted(bounds)
    sc, act = np.zeros((0, 2), np.float32), np.zeros((0, 2), np.uint8)
    for t0, t1 in zip(bounds[:-1], bounds[1:]):
        a, s, _ = detect_device(seg, _chunks(), receptive_field(), TASKS, onset=ONSET, offset=OFFSET, want_scores=True,
                                frame_range=(t0, t1), entry=act[-1] if t0 > 0 else None)
        assert a.shape == s.shape == (t1 - t0, 2)
        sc, act = np.concatenate([sc, s]), np.concatenate([act, a])
    return sc, act


def assert_same(got, ref):
    assert got[0].shape == ref[0].shape and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(got[1], ref[1])


def between_runs(y):
    """[(a, b)]: maximal runs of frames a .. b - 1 (a >= 1) that are not decisive (offset <= y <= onset)"""
    mid = (y >= np.float32(OFFSET)) & (y <= np.float32(ONSET))
    mid[0] = False
    d = np.diff(np.concatenate([[0], mid.astype(np.int8), [0]]))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


@pytest.mark.parametrize("Cn", [23, 1, 200])
def test_ranges_cut_at_window_starts_and_after_frame_zero(built_lib, gpu, Cn):
    """C = 23: T = 321, fewer frames than scan threads; C = 1; C = 200: T = 2091, more than 1024 and no multiple of 256"""
    seg, sc, act, starts, T = reference(gpu, Cn)
    assert T == {23: 321, 1: 101, 200: 2091}[Cn]
    assert_same(run_ranges(seg, [1], T), (sc, act))                                  # [0, 1), then the rest
    assert_same(run_ranges(seg, sorted(set(starts[1:].tolist())), T), (sc, act))     # a cut at every window start frame
    assert_same(run_ranges(seg, [T // 2, T // 2, T - 1], T), (sc, act))              # an empty range, a last single frame
    assert_same(run_ranges(seg, [], T), (sc, act))                                   # the range [0, T) itself


@pytest.mark.parametrize("Cn", [23, 200])
def test_single_frames_across_a_crossing_and_cuts_inside_undecided_runs(built_lib, gpu, Cn):
    seg, sc, act, starts, T = reference(gpu, Cn)
    states = set()
    for k in range(2):
        flips = np.nonzero(np.diff(act[:, k].astype(np.int8)) != 0)[0] + 1
        assert len(flips) >= 2, "the input has no threshold crossing"
        for t in (int(flips[0]), int(flips[len(flips) // 2])):
            lo, hi = max(t - 3, 1), min(t + 3, T - 1)
            assert_same(run_ranges(seg, list(range(lo, hi + 1)), T), (sc, act))      # [lo, lo+1), ... single frames over t
        runs = [r for r in between_runs(sc[:, k]) if r[1] - r[0] >= 2]
        assert runs, "the input has no run of frames between the thresholds"
        on = [r for r in runs if act[r[0], k] == 1]
        off = [r for r in runs if act[r[0], k] == 0]
        states.update(act[r[0], k] for r in runs)
        for a, b in on[:1] + off[:1] + [max(runs, key=lambda r: r[1] - r[0])]:
            assert_same(run_ranges(seg, [(a + b) // 2], T), (sc, act))               # a cut inside the run
            assert_same(run_ranges(seg, [a, a + 1, b], T), (sc, act))                # the run alone, entered twice
    assert states == {0, 1}, "undecided runs in both states are needed: the carried state must matter"


def test_range_without_decisive_frame_inherits_the_entry_state(built_lib, gpu):
    from diarizen_amd.postprocess import detect_device, receptive_field
    seg, sc, act, starts, T = reference(gpu, 23)
    # frames undecided in BOTH columns
    both = (sc >= np.float32(OFFSET)).all(1) & (sc <= np.float32(ONSET)).all(1)
    both[0] = False
    idx = np.nonzero(both[:-1] & both[1:])[0]
    assert len(idx), "the input has no two consecutive frames undecided in both columns"
    a = int(idx[0])
    for entry in ([0, 0], [1, 1], [1, 0], [0, 1]):
        got, s, _ = detect_device(seg, _chunks(), receptive_field(), TASKS, onset=ONSET, offset=OFFSET, want_scores=True,
                                  frame_range=(a, a + 2), entry=np.array(entry, np.uint8))
        assert np.array_equal(got, np.array([entry, entry], np.uint8))
        assert np.array_equal(s.view(np.uint32), sc[a:a + 2].view(np.uint32))
    # the launcher on device operands (what DetectionStream calls), from frame 0: no entry state
    import torch
    from diarizen_amd.postprocess import detect_range_launch, detection_weights
    d_start = torch.from_numpy(starts).to(gpu)
    d_w = torch.from_numpy(detection_weights(99, 2.0)).to(gpu)
    s2, _ = detect_range_launch(seg, 23, d_start, d_w, 0, 7, TASKS, ONSET, OFFSET, None)
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), sc[:7].view(np.uint32))


def test_abi_rejects_bad_ranges_and_launches_nothing(built_lib, gpu):
    import torch
    lib = built_lib
    seg, sc_ref, act_ref, starts, T = reference(gpu, 23)
    start = torch.from_numpy(starts).to(gpu)
    w = torch.ones(99, dtype=torch.float64, device=gpu)
    entry = torch.zeros(2, dtype=torch.uint8, device=gpu)
    sc = torch.full((40, 2), -7.0, dtype=torch.float32, device=gpu)
    act = torch.full((40, 2), 9, dtype=torch.uint8, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(t0, t1, entry_=True, sc_=True, act_=True, tasks=3, onset=ONSET, offset=OFFSET, S=4):
        return lib.dzn_detect_range(p(seg), 23, 99, S, p(start), p(w), t0, t1, tasks, onset, offset,
                                    p(entry) if entry_ else None, p(sc) if sc_ else None, p(act) if act_ else None, st)
    for args, kw in (((-1, 5), {}), ((10, 9), {}), ((5, 10), dict(entry_=False)), ((5, 10), dict(entry_=False, act_=False)),
                     ((0, 10), dict(sc_=False)), ((0, 10), dict(tasks=0)), ((0, 10), dict(tasks=4)),
                     ((0, 10), dict(onset=0.3, offset=0.7)), ((0, 10), dict(S=9))):
        assert call(*args, **kw) == -1, (args, kw)
    assert call(12, 12) == 0 and call(0, 0, entry_=False) == 0                      # empty: DZN_OK, no launch
    torch.cuda.synchronize()
    assert float(sc.min()) == -7.0 == float(sc.max()) and int(act.min()) == 9 == int(act.max())
    assert call(0, 10, entry_=False) == 0                                           # t0 == 0 needs no entry state
    torch.cuda.synchronize()
    assert int(act[:10].max()) <= 1 and int(act[10:].min()) == 9 and float(sc[10:].max()) == -7.0
