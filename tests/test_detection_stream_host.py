"""The committed prefix of a detection stream (diarizen_amd/detection.py, DetectionStream) on the CPU: with windows
0 .. C' - 1 computed, every frame before postprocess.committed_frames(C') — the start frame of window C' — has the scores and
the hysteresis output of the whole recording, bit for bit, and the frame AT that bound does not (the bound is tight); and the
frontier never runs past what the offline path computes for the recording, whatever its final length."""
import os

import numpy as np
import pytest

from diarizen_amd.core import SlidingWindow
from diarizen_amd.inference import window_plan
from diarizen_amd.postprocess import (_frame_grid, _hysteresis, committed_frames, crop_end, detection_scores_host,
                                      receptive_field)
from diarizen_amd.streaming import complete_windows

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "detection_ref.npz"))
# every decision array of the goldens but the 30-min one (2241 windows: the numpy aggregate over each of its prefixes is
# minutes of Python loop; its geometry, 8 s windows at ratio 0.1, is EN2002a's)
CASES = [str(c) for c in G["cases"] if str(c) != "host30"] + ["blocky"]
ONSET, OFFSET = 0.7, 0.3


def blocky(seed=11, C=23, L=99, S=4):
    """per (window, speaker) runs that toggle with probability 6 % per frame"""
    g = np.random.default_rng(seed)
    tog = g.random((C, L, S)) < 0.06
    tog[:, 0, :] = g.random((C, S)) < 0.4
    return (np.cumsum(tog, axis=1) % 2).astype(np.uint8)


def case(name):
    if name == "blocky":
        return blocky(), SlidingWindow(start=0.0, duration=2.0, step=0.1 * 2.0)
    src = str(G[f"{name}_src"])
    if src == "here":
        seg = G[f"{name}_seg"]
    else:
        f, key = src.split(":")
        seg = np.load(os.path.join(GOLD, f))[key]
    dur, ratio, _ = G[f"{name}_args"]
    return seg, SlidingWindow(start=0.0, duration=float(dur), step=float(ratio) * float(dur))


def test_committed_frames_is_the_start_frame_of_the_next_window():
    frames = receptive_field()
    for dur, ratio in ((2.0, 0.1), (2.0, 0.5), (5.0, 0.5), (8.0, 0.1)):
        chunks = SlidingWindow(start=0.0, duration=dur, step=ratio * dur)
        _, starts, _ = _frame_grid(300, 99, chunks, frames)
        assert [committed_frames(c, chunks, frames) for c in range(300)] == starts.tolist()
        assert committed_frames(0, chunks, frames) == 0
        # start frames do not depend on the number of windows
        assert np.array_equal(_frame_grid(7, 99, chunks, frames)[1], starts[:7])


@pytest.mark.parametrize("name", CASES)
def test_prefix_of_windows_gives_the_final_bits_before_the_frontier(name):
    seg, chunks = case(name)
    frames = receptive_field()
    C = len(seg)
    tight = 0
    for task in (1, 2):
        full = detection_scores_host(seg, chunks, frames, task).data[:, 0]
        full_act = _hysteresis(full, ONSET, OFFSET)
        for c in range(1, C + 1):
            F = committed_frames(c, chunks, frames)
            part = detection_scores_host(seg[:c], chunks, frames, task).data[:, 0]
            assert F < len(part) or c == C
            F = min(F, len(part))
            assert np.array_equal(part[:F].view(np.uint32), full[:F].view(np.uint32)), (name, task, c)
            assert np.array_equal(_hysteresis(part, ONSET, OFFSET)[:F], full_act[:F]), (name, task, c)
            if c < C and part[F].view(np.uint32) != full[F].view(np.uint32):
                tight += 1
    if C > 1:
        assert tight > 0, "no prefix whose first uncommitted frame differs: the bound would not be tight"


@pytest.mark.parametrize("duration,ratio", [(8.0, 0.1), (2.0, 0.1), (2.0, 0.5)])
def test_frontier_stays_inside_the_offline_output(duration, ratio):
    """recording lengths over one whole step in samples around the completion of window 1, 2 and 5: at every earlier feed
    point (every number of complete windows up to the final one) the frontier is at most the number of frames the offline
    path keeps for that length (detection.apply: _frame_grid, crop_end when the last window is zero-padded)"""
    sr = 16000
    frames = receptive_field(sr)
    chunks = SlidingWindow(start=0.0, duration=duration, step=ratio * duration)
    window, step = int(np.floor(duration * sr)), int(round(ratio * duration * sr))
    L = 99
    front = [committed_frames(c, chunks, frames) for c in range(8)]
    assert front == sorted(front)
    for k in (1, 2, 5):
        mid = window + (k - 1) * step
        for n in range(max(1, mid - step // 2), mid + step // 2 + 1):
            n_full, has_last = window_plan(n, window, step)
            grid, _, T = _frame_grid(n_full + int(has_last), L, chunks, frames)
            if has_last:
                T = crop_end(T, grid, n / sr)
            c = complete_windows(n, window, step)              # feed points n' <= n have at most this many
            assert c == n_full
            assert front[c] <= T, (n, c, front[c], T)
