"""The host bookkeeping of a session with a committed prefix (diarizen_amd/streaming.py, StreamRows), without a device: the rows
grow by doubling and keep what they held, the span of a range step is clamped, the committed rows are copies that never shrink.
And the one statement of the frame arithmetic (postprocess.covered_frames) against _frame_grid and the numpy aggregate."""
import numpy as np

from diarizen_amd.core import SlidingWindow
from diarizen_amd.postprocess import _frame_grid, aggregate, covered_frames, receptive_field
from diarizen_amd.streaming import StreamRows

K = 3


def rows():
    return StreamRows(act=(np.uint8, (K,)), sc=(np.float32, (K,)), cnt=(np.uint8, ()))


def block(t0, t1):
    """rows t0 .. t1 - 1 of three arrays whose every element names its row (and column)"""
    t = np.arange(t0, t1)
    return dict(act=((t[:, None] + np.arange(K)) % 251).astype(np.uint8), sc=(t[:, None] + 0.25 * np.arange(K)).astype(np.float32),
                cnt=(t % 7).astype(np.uint8))


def step(r, upto, frontier):
    """one range step as CommittedStream._advance makes it; -> the span it computed"""
    t0, t1, f = r.span(upto, frontier)
    r.write(t0, t1, f, **(block(t0, t1) if t1 > t0 else {}))
    return t0, t1, f


def test_rows_grow_by_doubling_and_keep_earlier_rows():
    r = rows()
    assert (r.frontier, r.covered) == (0, 0) and len(r.valid("act")) == 0 and len(r.committed("cnt")) == 0
    caps = []
    for upto in (1000, 1030, 5000):                 # inside the first 1024 rows, across them, more than a doubling
        t0, t1, f = step(r, upto, upto)
        assert (t1, f, r.frontier, r.covered) == (upto, upto, upto, upto)
        caps.append(len(r._rows["act"]))
        want = block(0, upto)
        for name, a in want.items():
            got = r.valid(name)
            assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a)
            assert all(len(v) == caps[-1] for v in r._rows.values())
    assert caps == [1024, 2048, 5000]               # max(t1, 2 * len)
    assert r.valid("act").shape == (5000, K) and r.valid("sc").shape == (5000, K) and r.valid("cnt").shape == (5000,)


def test_span_is_clamped():
    r = rows()
    step(r, 300, 200)                               # 200 committed, 100 provisional
    assert (r.frontier, r.covered) == (200, 300)
    # t1 < t0: nothing to compute, nothing moves back
    assert r.span(150, 150) == (200, 200, 200)
    before = r.valid("act").copy()
    assert step(r, 150, 150) == (200, 200, 200)
    assert (r.frontier, r.covered) == (200, 200) and np.array_equal(r.valid("act"), before[:200])
    # a frontier below t0 is raised to t0, one above t1 lowered to t1
    assert r.span(400, 120) == (200, 400, 200)
    assert r.span(400, 999) == (200, 400, 400)
    assert step(r, 400, 999) == (200, 400, 400)
    assert (r.frontier, r.covered) == (400, 400)
    assert np.array_equal(r.valid("cnt"), block(0, 400)["cnt"])


def test_committed_rows_are_copies_that_never_shrink():
    r = rows()
    prev = {k: r.committed(k) for k in ("act", "sc", "cnt")}
    for upto, frontier in ((500, 360), (540, 400), (540, 380), (1500, 1400), (1400, 1300), (3000, 3000)):
        step(r, upto, frontier)
        for k, p in prev.items():
            c = r.committed(k)
            assert len(c) == r.frontier >= len(p) and np.array_equal(c[:len(p)], p)
            assert np.array_equal(c, block(0, r.frontier)[k])
            c[...] = 0                              # a copy: writing to it changes nothing
            assert np.array_equal(r.committed(k), block(0, r.frontier)[k])
            prev[k] = r.committed(k)
        assert r.frontier <= r.covered


def test_covered_frames_is_the_length_of_the_frame_grid_and_of_aggregate():
    frames = receptive_field()
    L = 99
    for dur, ratio in ((2.0, 0.1), (2.0, 0.5), (5.0, 0.5), (8.0, 0.1)):
        chunks = SlidingWindow(start=0.0, duration=dur, step=ratio * dur)
        for C in range(1, 301):
            assert covered_frames(C, chunks, frames) == _frame_grid(C, L, chunks, frames)[2]
        for C in (1, 2, 3, 7, 50, 300):             # the reference restatement itself
            assert covered_frames(C, chunks, frames) == len(aggregate(np.zeros((C, L, 1), np.float32), chunks, frames).data)
