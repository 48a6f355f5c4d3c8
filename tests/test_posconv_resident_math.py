"""The arithmetic csrc/posconv_resident.hip states in its header, walked over every case (CPU): the bank arithmetic of the
resident rows' LDS image at ANY row offset, and the span of padded rows a 256-row tile's taps touch."""
from test_design_math import _worst_conflict, _wswz

BM = 256


def _rswz(row):   # posconv_resident.hip: rswz
    return (row >> 1) & 3


def test_resident_rows_are_conflict_free_at_every_row_offset():
    """lane (lr = l & 15, lq = l >> 4) reads chunk lq of LDS row R + lr, stored at slot lq ^ key(row) of the row's 64 bytes"""
    for R in range(0, 160):
        a = lambda l: (R + (l & 15)) * 64 + (((l >> 4) ^ _rswz(R + (l & 15))) << 4)
        assert _worst_conflict(a) == 1, R


def test_the_aligned_tiles_key_is_not_offset_free():
    """why the resident image does not keep pswz: conflict free at multiples of 16 rows (all the staged tiles need), two-way at
    offsets in between"""
    worst = {}
    for R in range(0, 64):
        w = lambda l: (R + (l & 15)) * 64 + (((l >> 4) ^ _wswz(R + (l & 15))) << 4)
        worst[R] = _worst_conflict(w)
    assert all(worst[R] == 1 for R in range(0, 64, 16))
    assert max(worst.values()) == 2


def test_kernel_does_not_spill_and_keeps_two_wavefronts_per_simd():
    """hipcc's resource report for csrc/posconv_resident.hip: ScratchSize 0, and registers that leave the workgroup's 8
    wavefronts two per SIMD (at most 256 VGPRs + AGPRs)"""
    import os
    import re
    import shutil
    import subprocess
    import pytest
    from diarizen_amd import build as b
    if not shutil.which(b.HIPCC) and not os.path.exists(b.HIPCC):
        pytest.skip("hipcc not available")
    r = subprocess.run([b.HIPCC, *b.FLAGS, "-c", str(b.CSRC / "posconv_resident.hip"), "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]
    mine = [blk for blk in blocks if "posconv_resident_kernel" in blk.split()[0]]
    assert len(mine) == 1
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1))
    regs = int(re.search(r" VGPRs: (\d+)", mine[0]).group(1)) + int(re.search(r"AGPRs: (\d+)", mine[0]).group(1))
    occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", mine[0]).group(1))
    assert scratch == 0 and regs <= 256 and occ >= 2, (scratch, regs, occ)


def _span(B, L, Kc):   # posconv_resident.hip: posconv_span
    nb = min((L + BM - 2) // L, B - 1)
    return BM - 1 + Kc * (1 + nb)


def test_span_covers_every_tile():
    """LDS row of output row m at tap j: prow(m) + j - prow(m0), prow(m) = m + (m // L) Kc; the largest over a tile's rows and
    taps stays below posconv_span, and the bound is reached by some shape (it is not slack by construction)"""
    tight = False
    for Kc in (1, 16, 128):
        for L in (1, 2, 15, 79, 80, 81, 127, 128, 129, 255, 256, 257, 399, 600):
            for B in (1, 2, 3, 7):
                M, span = B * L, _span(B, L, Kc)
                for m0 in range(0, M, BM):
                    m1 = min(m0 + BM, M) - 1
                    top = (m1 + (m1 // L) * Kc) - (m0 + (m0 // L) * Kc) + Kc - 1
                    assert top < span, (Kc, L, B, m0)
                    tight = tight or top == span - 1
    assert tight
    assert _span(561, 399, 128) == 511          # the model's shape: 512 rows x 256 B = 128 KB resident
