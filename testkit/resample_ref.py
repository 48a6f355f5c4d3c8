"""Float64 reference of the polyphase resampler and the fp32 dot-product bound that the resampler tests share
(tests/test_resample_host.py, tests/test_resample_gpu.py)."""
from __future__ import annotations

import numpy as np

# (input rate, T) -> 16 kHz: T = 1, T shorter than `width`, T no multiple of o, upsampling (8 kHz), even o (32 kHz)
CASES = [(48000, 4800), (44100, 22050), (44100, 1001), (22050, 5000), (8000, 777), (32000, 3001), (44100, 1), (48000, 5)]


def case_input(rate: int, T: int) -> np.ndarray:
    """0.3 * randn, float32, seeded by the case"""
    return (0.3 * np.random.default_rng(rate * 7 + T).standard_normal(T)).astype(np.float32)


def reference(x32: np.ndarray, bank: np.ndarray, o: int, n: int, width: int):
    """-> (ref, mag), float64 [ceil(n T / o)]:  ref[m] = sum_j float64(bank[p, j]) * float64(x32[f o + j - width]) with
    m = f n + p and x = 0 outside the recording, and mag[m] the same sum over the absolute values.  An fp32 dot product of
    K terms, in any order, with or without fused multiply-adds, is within K * 2^-24 * mag[m] of ref[m]."""
    T, K = len(x32), bank.shape[1]
    M = -((-n * T) // o)
    F = -(-M // n)
    xp = np.zeros(width + (F - 1) * o + K + T, dtype=np.float64)
    xp[width:width + T] = x32
    win = np.lib.stride_tricks.as_strided(xp, shape=(F, K), strides=(o * xp.strides[0], xp.strides[0]), writeable=False)
    b64 = bank.astype(np.float64)
    ref = (win @ b64.T).reshape(-1)[:M]
    mag = (np.abs(win) @ np.abs(b64).T).reshape(-1)[:M]
    return ref, mag


def assert_within_bound(y: np.ndarray, ref: np.ndarray, mag: np.ndarray, K: int, what: str = ""):
    """every output sample: |y - ref| <= K 2^-24 mag, and y == 0 exactly where mag == 0; prints the worst ratio"""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == ref.shape, f"{what}: length {y.shape} != {ref.shape}"
    bound = K * 2.0 ** -24 * mag
    err = np.abs(y - ref)
    nz = mag > 0
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print(f"{what}: worst |y - ref| / bound = {worst:.3f} over {len(y)} samples")
    assert np.all(y[~nz] == 0.0), f"{what}: non-zero output where every product is zero"
    assert np.all(err <= bound), f"{what}: worst |y - ref| / bound = {worst:.3f}"
