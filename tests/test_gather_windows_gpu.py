"""dzn_gather_windows (csrc/ingest.hip, ops.gather_windows) on the MI355X: dst[b, :] = pool[offsets[b] : offsets[b] + window]
for one and for 65 windows of 1 .. 128000 samples, offsets of all four alignments mod 4 in different rows of the pool —
the 16-byte path where source and destination rows are both aligned, the scalar path elsewhere — including a window that
reaches into a row's zero tail; torch.equal to torch indexing.  No windows: no launch.  A window that leaves the pool is
refused on the host."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW, ROWS, FILLED = 140000, 3, 135000               # rows of 140000 floats, zeros from 135000 on


@pytest.fixture(scope="module")
def pool(built_lib, gpu):
    g = torch.Generator().manual_seed(7)
    p = torch.randn((ROWS, ROW), generator=g)
    p[:, FILLED:] = 0.0
    return p.to(gpu)


def offsets_for(B: int, window: int) -> np.ndarray:
    """B offsets: every alignment mod 4, every row, the last one as far into the row's zero tail as the row allows"""
    room = ROW - window
    g = np.random.default_rng(1000 * B + window)
    off = [(b % ROWS) * ROW + min(room, 4 * int(g.integers(0, room // 4 + 1)) + b % 4) for b in range(B)]
    off[-1] = (ROWS - 1) * ROW + room                # ends with the pool
    return np.array(off, dtype=np.int64)


@pytest.mark.parametrize("window", [1, 3, 4, 1023, 128000])
@pytest.mark.parametrize("B", [1, 65])
def test_gather_equals_torch_indexing(gpu, pool, B, window):
    from diarizen_amd import ops
    off = offsets_for(B, window)
    if B > 1:
        assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3} and {int(o) // ROW for o in off} == set(range(ROWS))
    flat = pool.view(-1)
    want = torch.stack([flat[int(o):int(o) + window] for o in off])
    out = torch.full((B, window), float("nan"), device=gpu)
    got = ops.gather_windows(pool, off, window, out=out)
    assert got is out and torch.equal(got, want)
    if window == 128000:
        assert bool((got[-1, FILLED - (ROW - window):] == 0).all()) and bool(got[-1, :100].abs().sum() > 0)      # the zero tail
    # an unaligned destination: the same windows into a view that starts one float into a larger buffer
    big = torch.full((B * window + 1,), float("nan"), device=gpu)
    got = ops.gather_windows(pool, off, window, out=big[1:].view(B, window))
    assert torch.equal(got, want) and bool(torch.isnan(big[0]))


def test_no_windows_is_a_no_op_and_a_window_outside_the_pool_is_refused(gpu, pool):
    from diarizen_amd import _lib, ops
    _lib.profile_enable(True)
    try:
        _lib.profile_collect()
        out = ops.gather_windows(pool, [], 128000)
        torch.cuda.synchronize()
        assert out.shape == (0, 128000) and not [e for e in _lib.profile_collect() if e["name"] == "gather_windows"]
    finally:
        _lib.profile_enable(False)
    out = torch.full((2, 1023), 5.0, device=gpu)
    for bad in ([0, ROWS * ROW - 1022], [-1, 0]):
        with pytest.raises(_lib.DznError, match="dzn_gather_windows: window [01] at float .* leaves the pool"):
            ops.gather_windows(pool, bad, 1023, out=out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
