"""Restatements of the GCC-PHAT delay-and-sum beamformer (csrc/beamform.hip) in numpy, and the inputs of its
tests.

  raw_delays(x, ref, hop, max_lag, dtype)  lag, peak and the margin between the best and the second-best correlation value over
                                           the search range, per (channel, block): dtype float64 is the reference, float32 the
                                           same statement on numpy's single-precision FFT (their peak difference sets the
                                           comparison margin of the device test)
  synth(x, delays, hop)                    the alignment pass in float32, operation by operation as the kernel does it
  case(name)                               the seeded inputs A .. E of the tests
"""
from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN_WAV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "EN2002a_30s.wav")


def num_blocks(T: int, hop: int) -> int:
    return -(-int(T) // int(hop)) + 1


def supported(T: int, hop: int) -> np.ndarray:
    """bool [nb]: the blocks whose frame holds at least `hop` samples of the recording"""
    b = np.arange(num_blocks(T, hop), dtype=np.int64)
    return np.minimum(T, (b + 1) * hop) - np.maximum(0, (b - 1) * hop) >= hop


def visiting_order(max_lag: int) -> np.ndarray:
    """0, -1, +1, -2, +2, .. , -L, +L"""
    k = np.arange(1, int(max_lag) + 1)
    return np.concatenate([[0], np.stack([-k, k], axis=1).reshape(-1)]).astype(np.int64)


def frames_of(x: np.ndarray, hop: int) -> np.ndarray:
    """[C, T] -> [nb, C, 2 hop]: frame b is samples (b - 1) hop .. (b + 1) hop - 1, zero outside the recording"""
    C, T = x.shape
    nb = num_blocks(T, hop)
    padded = np.zeros((C, (nb + 1) * hop), dtype=x.dtype)
    padded[:, hop:hop + T] = x
    return np.stack([padded[:, b * hop:(b + 2) * hop] for b in range(nb)])


def raw_delays(x, ref: int, hop: int, max_lag: int, dtype=np.float64):
    """x float32 [C, T] -> (lag int32 [C, nb], peak dtype [C, nb], margin dtype [C, nb]); the reference row is 0 / 0 / 0.
    Everything is computed in `dtype`: the Hann window comes from a float64 cosine rounded once, the transforms are numpy's
    (single precision for float32 input)."""
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    C, T = x.shape
    W = 2 * hop
    nb = num_blocks(T, hop)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)).astype(dtype)
    X = np.fft.fft(frames_of(x, hop) * window, axis=-1)                     # [nb, C, W]
    assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128), X.dtype
    P = X * np.conj(X[:, ref:ref + 1])
    mag = np.abs(P)
    G = np.where(mag > 0, P / np.where(mag > 0, mag, 1), 0).astype(X.dtype)
    g = np.fft.ifft(G, axis=-1).real                                        # [nb, C, W], circular
    assert g.dtype == dtype, g.dtype
    vals = g[..., visiting_order(max_lag) % W]                              # in visiting order: argmax keeps the first maximum
    best = np.argmax(vals, axis=-1)
    lag = visiting_order(max_lag)[best]
    top = np.sort(vals, axis=-1)
    peak, margin = top[..., -1], top[..., -1] - top[..., -2]
    lag, peak, margin = lag.T.astype(np.int32), np.ascontiguousarray(peak.T), np.ascontiguousarray(margin.T)
    lag[ref], peak[ref], margin[ref] = 0, 0, 0
    return lag, peak, margin


def synth(x, delays, hop: int) -> np.ndarray:
    """x float32 [C, T], delays int [C, nb] -> float32 [T]: S_b(n) = (x_0[n + d_0b] + x_1[n + d_1b] + ..) / C as a float32
    running sum in ascending channel order and one division, y[n] = a + w (v - a) with a = S_b(n), v = S_{b+1}(n),
    w = (n - b hop) / hop, each operation rounded to float32"""
    x = np.asarray(x, dtype=np.float32)
    d = np.asarray(delays, dtype=np.int64)
    C, T = x.shape
    assert d.shape == (C, num_blocks(T, hop)) and np.abs(d).max(initial=0) <= hop // 2
    pad = hop
    padded = np.zeros((C, T + 2 * pad), dtype=np.float32)
    padded[:, pad:pad + T] = x
    y = np.empty(T, dtype=np.float32)

    def mean_at(n, b):
        s = padded[0, pad + n + d[0, b]].copy()
        for c in range(1, C):
            s += padded[c, pad + n + d[c, b]]
        s /= np.float32(C)
        return s

    for b in range(num_blocks(T, hop) - 1):
        n = np.arange(b * hop, min(T, (b + 1) * hop), dtype=np.int64)
        if not len(n):
            break
        w = ((n - b * hop).astype(np.float32) / np.float32(hop)).astype(np.float32)
        a, v = mean_at(n, b), mean_at(n, b + 1)
        t = (v - a).astype(np.float32)
        t = (w * t).astype(np.float32)
        y[n] = a + t
    return y


def delayed_copies(s: np.ndarray, delays, sigma: float, seed: int) -> np.ndarray:
    """x_c[i] = s[i - d_c] (s = 0 outside its support) plus independent white noise of deviation sigma -> float32 [C, T]"""
    s = np.asarray(s, dtype=np.float32)
    T = len(s)
    g = np.random.default_rng(seed)
    x = np.zeros((len(delays), T), dtype=np.float32)
    for c, dc in enumerate(delays):
        if dc >= 0:
            x[c, dc:] = s[:T - dc]
        else:
            x[c, :T + dc] = s[-dc:]
        if sigma:
            x[c] += (sigma * g.standard_normal(T)).astype(np.float32)
    return x


def white(T: int, deviation: float, seed: int) -> np.ndarray:
    return (deviation * np.random.default_rng(seed).standard_normal(T)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden_10s() -> np.ndarray:
    return golden_wav()[:160000]


@functools.lru_cache(maxsize=None)
def golden_wav() -> np.ndarray:
    """float32 [480000]: the 30 s fixture (PCM16 mono, 16 kHz), sample * 2^-15 — read with the standard library, because
    testkit/ imports nothing from the product"""
    import wave
    with wave.open(GOLDEN_WAV, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 16000)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    x = pcm.astype(np.float32) * np.float32(2.0 ** -15)
    x.setflags(write=False)
    return x


_CASES = {
    # name: (source, T, delays, sigma, hop, max_lag)
    "A": ("white", 3 * 4096 + 77, (0, 3, -160, 160, 1, -1, 50, -99), 0.03, 4096, 160),
    "B": ("golden", 160000, (0, 7, -23, 112), 0.002, 4096, 160),
    "C": ("golden", 160000, (0, -5), 0.0, 4096, 160),
    "D": ("white", 5 * 256 + 1, (0, -8, 8, 2), 0.03, 256, 8),
    "E": ("white", 100, (0, 4), 0.0, 256, 8),
}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> dict(name, s float32 [T], x float32 [C, T], delays tuple, sigma, hop, max_lag), seeded and read-only"""
    kind, T, delays, sigma, hop, max_lag = _CASES[name]
    seed = 1000 + ord(name)
    s = golden_10s() if kind == "golden" else white(T, 0.1, seed)
    assert len(s) == T
    x = delayed_copies(s, delays, sigma, seed + 1)
    x.setflags(write=False)
    s.setflags(write=False)
    return dict(name=name, s=s, x=x, delays=delays, sigma=sigma, hop=hop, max_lag=max_lag)


@functools.lru_cache(maxsize=None)
def reference(name: str, ref: int = 0):
    """raw_delays of case `name` in float64 (computed once per process): (lag, peak, margin)"""
    c = case(name)
    out = raw_delays(c["x"], ref, c["hop"], c["max_lag"], np.float64)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def comparison_margin():
    """(E, m): E = the largest |peak_float32 - peak_float64| of the two numpy restatements over cases A .. E, m = 32 E — the
    device transform has another butterfly order and twiddle rounding than numpy's, its error shares the eps log2 W scale, and
    32 x leaves room for constant factors"""
    E = 0.0
    for name in _CASES:
        c = case(name)
        p32 = raw_delays(c["x"], 0, c["hop"], c["max_lag"], np.float32)[1]
        E = max(E, float(np.abs(p32.astype(np.float64) - reference(name)[1]).max()))
    return E, 32.0 * E
