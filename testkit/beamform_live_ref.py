"""The causal delay rule of live array feeds (csrc/beamform_live.hip) restated as plain loops, the feed
schedule, and the inputs of its tests.  testkit/beamform_ref.py holds what the rule is applied to (raw_delays, synth).

  causal_delays(lag, peak, T, hop, min_peak, ref)   the rule, block by block, with no numpy idiom the product could share
  beam_ready(R, hop)                                the beamformed samples that are final after R frames
  piecewise(s, segments, sigma, seed, gaps)         a source copied into channels whose delays change from segment to segment
  signal(name)                                      the seeded signals P, Q, R
"""
from __future__ import annotations

import functools

import numpy as np

from . import beamform_ref


def causal_delays(lag, peak, T: int, hop: int, min_peak: float, ref: int = 0) -> np.ndarray:
    """int [C, nb] lags, float32 [C, nb] peaks -> int32 [C, nb]"""
    lag = np.asarray(lag)
    peak = np.asarray(peak, dtype=np.float32)
    C, nb = lag.shape
    assert nb == beamform_ref.num_blocks(T, hop) and peak.shape == lag.shape
    floor = np.float32(min_peak)
    out = np.zeros((C, nb), dtype=np.int32)
    for c in range(C):
        if c == ref:
            continue
        held = []
        for b in range(nb):
            samples = min(T, (b + 1) * hop) - max(0, (b - 1) * hop)
            if samples >= hop and peak[c, b] >= floor:
                held.append(int(lag[c, b]))
            else:
                held.append(held[-1] if held else 0)
            five = [held[k] if k >= 0 else held[0] for k in range(b - 4, b + 1)]
            out[c, b] = sorted(five)[2]
    return out


def beam_ready(frames: int, hop: int) -> int:
    return max(0, frames // hop - 1) * hop


def piecewise(s, segments, sigma: float, seed: int, gaps) -> np.ndarray:
    """s float32 [T]; segments = ((start, (d_0, d_1, ..)), ..) in ascending start, the first at 0: x_c[i] = s[i - d_c] with the
    delays of the segment that holds i (s = 0 outside its support), plus independent white noise of deviation sigma; then the
    channels 1 .. are set to exactly zero on every gap [a, z).  -> the values an int16 feed delivers: round(x 2^15) 2^-15,
    float32 [C, T] (with the int16 frames: `frames_of`)"""
    s = np.asarray(s, dtype=np.float32)
    T = len(s)
    C = len(segments[0][1])
    x = np.zeros((C, T), dtype=np.float32)
    bounds = [a for a, _ in segments[1:]] + [T]
    for (a, delays), z in zip(segments, bounds):
        a, z = min(a, T), min(z, T)
        x[:, a:z] = beamform_ref.delayed_copies(s, delays, 0.0, 0)[:, a:z]
    g = np.random.default_rng(seed)
    x += (sigma * g.standard_normal((C, T))).astype(np.float32)
    for a, z in gaps:
        x[1:, min(a, T):min(z, T)] = 0.0
    pcm = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return pcm.astype(np.float32) * np.float32(2.0 ** -15)


def frames_of(x: np.ndarray) -> np.ndarray:
    """float32 [C, T] of `piecewise` -> the interleaved int16 frames [T, C] it was decoded from"""
    pcm = np.asarray(x, dtype=np.float64).T * 32768.0
    assert np.array_equal(pcm, np.rint(pcm))
    return np.ascontiguousarray(pcm.astype(np.int16))


_SIGNALS = {
    # name: (hop, max_lag, T)
    "P": (256, 8, 14 * 256 + 37),
    "Q": (256, 8, 14 * 256),
    "R": (512, 24, 14 * 512 + 3),
}
REFERENCE = 0


@functools.lru_cache(maxsize=None)
def signal(name: str):
    """-> dict(name, x float32 [4, T], hop, max_lag, T, min_peak), seeded and read-only"""
    hop, max_lag, T = _SIGNALS[name]
    s = beamform_ref.white(T, 0.1, 7 + hop)
    segments = ((0, (0, 3, -8, 8)), (4 * hop + 17, (0, -2, 5, 8)), (11 * hop, (0, -2, 5, -7)))
    gaps = ((0, 2 * hop + 5), (13 * hop // 2, 19 * hop // 2))
    x = piecewise(s, segments, 0.01, 11 + hop, gaps)
    x.setflags(write=False)
    return dict(name=name, x=x, hop=hop, max_lag=max_lag, T=T, min_peak=8.0 / float(np.sqrt(2.0 * hop)))


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(lag, peak, margin) of signal `name` in float64 (beamform_ref.raw_delays; computed once per process)"""
    c = signal(name)
    out = beamform_ref.raw_delays(c["x"], REFERENCE, c["hop"], c["max_lag"], np.float64)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_delays(name: str) -> np.ndarray:
    """the causal delays of signal `name` from its float64 lags and peaks"""
    c = signal(name)
    lag, peak, _ = reference(name)
    d = causal_delays(lag, peak.astype(np.float32), c["T"], c["hop"], c["min_peak"], REFERENCE)
    d.setflags(write=False)
    return d


def random_case(seed: int = 5, C: int = 4, nb: int = 23, hop: int = 256, max_lag: int = 8):
    """random lags and peaks [C, nb] of a recording whose last block is unsupported: the peaks straddle float32(min_peak) —
    the value itself and its two float32 neighbours included — so that about half of the blocks are unreliable
    -> (lag int32, peak float32, T, hop, min_peak)"""
    g = np.random.default_rng(seed)
    T = (nb - 2) * hop + 9                              # the last frame holds 9 samples
    assert beamform_ref.num_blocks(T, hop) == nb and not beamform_ref.supported(T, hop)[-1]
    min_peak = 8.0 / float(np.sqrt(2.0 * hop))
    floor = np.float32(min_peak)
    lag = g.integers(-max_lag, max_lag + 1, size=(C, nb)).astype(np.int32)
    peak = (floor * g.uniform(0.5, 1.5, size=(C, nb))).astype(np.float32)
    edge = [floor, np.nextafter(floor, np.float32(0)), np.nextafter(floor, np.float32(1))]
    for c in range(C):
        at = g.choice(nb - 1, size=3, replace=False)
        peak[c, at] = edge
    peak[:, -1] = 1.0                                   # high and meaningless: the support rule must hold it back
    return lag, peak, T, hop, min_peak
