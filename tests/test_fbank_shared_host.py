"""The runner's side of the shared fbank: which windows go to dzn_embed_forward_strided, when its
frame grid is shared, and the index arithmetic b q + t of that grid.  No GPU: the functions are plain integer code."""
import pytest

from diarizen_amd.inference import (FBANK_FRAME, FBANK_SHIFT, embed_routes, fbank_frames, fbank_grid, fbank_is_shared,
                                    window_plan)

GEOMETRIES = [(2000, 160), (2000, 320), (2000, 800), (2000, 1760), (128000, 12800), (256000, 25600), (400, 160), (560, 320)]


@pytest.mark.parametrize("window,stride", GEOMETRIES)
@pytest.mark.parametrize("B", [1, 2, 3, 11])
def test_window_rows_cover_the_frame_grid_without_gaps(window, stride, B):
    """rows b q + t, b < B, t < T, are exactly 0 .. G - 1, and row b q + t holds the very samples of window b's frame t"""
    q, T, G = fbank_grid(B, window, stride)
    assert T == fbank_frames(window) and q * FBANK_SHIFT == stride
    rows = {b * q + t for b in range(B) for t in range(T)}
    assert rows == set(range(G))
    for b in range(B):
        for t in (0, T // 2, T - 1):
            first = b * stride + t * FBANK_SHIFT                 # first sample of window b's frame t, in the recording
            assert first == (b * q + t) * FBANK_SHIFT            # = first sample of recording frame b q + t
            assert first + FBANK_FRAME <= (B - 1) * stride + window      # inside the span the windows cover


def test_both_stride_conditions():
    N = 2000
    T = fbank_frames(N)
    assert T == 11
    for s in (160, 320, 800, 1760):
        assert fbank_is_shared(N, s)
    assert N - FBANK_FRAME + FBANK_SHIFT == 1760 and 1760 // FBANK_SHIFT == T     # the largest gap-free stride: q == T
    assert not fbank_is_shared(N, 1920)          # a multiple of the shift, but frame 11 of the grid belongs to no window
    assert not fbank_is_shared(N, N)             # unrelated (dense) windows
    assert not fbank_is_shared(N, 801) and not fbank_is_shared(N, 159)      # not whole frame shifts
    assert not fbank_is_shared(N, 0) and not fbank_is_shared(N, -160)
    assert fbank_is_shared(128000, 12800) and fbank_grid(561, 128000, 12800) == (80, 798, 560 * 80 + 798)
    # every step ratio of 0.1 over whole seconds of 16 kHz audio is a whole number of shifts
    for seconds in (2, 4, 8, 16):
        assert fbank_is_shared(seconds * 16000, seconds * 1600)


@pytest.mark.parametrize("num_samples", [128000, 128000 + 12800 * 7, 128000 + 12800 * 7 + 1, 200000, 90000, 399])
def test_padded_last_window_takes_the_dense_entry(num_samples):
    """the runner's batches: windows of the recording go to the strided entry, the zero-padded last window of
    window_plan (it does not lie in the recording) to the dense one, and every window goes to exactly one of them"""
    window, step, bs = 128000, 12800, 3
    n_full, has_last = window_plan(num_samples, window, step)
    C = n_full + int(has_last)
    dense_from = n_full if has_last else C
    strided, dense = [], []
    for s0 in range(0, C, bs):
        s1 = min(s0 + bs, C)
        ns, nd = embed_routes(s0, s1, dense_from)
        assert ns >= 0 and nd >= 0 and ns + nd == s1 - s0
        strided += list(range(s0, s0 + ns))
        dense += list(range(s0 + ns, s1))
    assert strided == list(range(n_full))
    assert dense == ([n_full] if has_last else [])
    for c in strided:
        assert c * step + window <= num_samples                  # wholly inside the recording
    for c in dense:
        assert c * step + window > num_samples


def test_routes_of_a_window_range():
    assert embed_routes(4, 8, 10) == (4, 0)
    assert embed_routes(8, 11, 10) == (2, 1)
    assert embed_routes(10, 11, 10) == (0, 1)
    assert embed_routes(0, 1, 0) == (0, 1)
