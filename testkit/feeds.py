"""Shared by the live-feed tests (tests/test_feed_format_host.py, tests/test_decode_gpu.py, tests/test_feed_ingest_gpu.py,
tests/test_feed_sessions_gpu.py): every stored format of the same seeded frames with what the host decoders make of them
(`stored_forms`, restating the helper of tests/test_telephony_gpu.py), the chunkings a feed loop is tried with, and a float64
model of one planned call that sees ONLY the bytes the call uploads.  numpy and audioop only: nothing here imports diarizen_amd,
and nothing under diarizen_amd/ imports this."""
from __future__ import annotations

import audioop

import numpy as np

from .telephony import all_codes

# (rate, frames, channels): the telephony tests' shapes (two full resample tiles plus a ragged third; o = 1 n = 2; o = 3
# n = 1; even o with an odd channel count; o = 441 n = 640) and 44.1 kHz, whose first outputs appear only after 458 frames
SHAPES = [(8000, 1500, 2), (48000, 7200, 2), (32000, 5001, 3), (11025, 1700, 1), (44100, 3001, 1)]


def stored_forms(T: int, C: int, seed: int):
    """name -> (stored array, float32 [C, T] that the host decoders make of it), for every stored format"""
    codes256 = bytes(range(256))                                        # the G.711 tables, from audioop
    ulaw_table = np.frombuffer(audioop.ulaw2lin(codes256, 2), dtype="<i2")
    alaw_table = np.frombuffer(audioop.alaw2lin(codes256, 2), dtype="<i2")
    g = np.random.default_rng(seed)
    forms = {}
    s16 = g.integers(-32768, 32768, size=(T, C)).astype(np.int16)
    forms["s16"] = (s16, s16.astype(np.float32) * np.float32(2.0 ** -15))
    u8 = g.integers(0, 256, size=(T, C)).astype(np.uint8)
    u8.reshape(-1)[:2] = (0, 255)
    forms["u8"] = (u8, (u8.astype(np.float32) - 128.0) / 128.0)
    v24 = g.integers(-2 ** 23, 2 ** 23, size=(T, C)).astype(np.int32)
    v24.reshape(-1)[:2] = (-2 ** 23, 2 ** 23 - 1)
    b24 = np.ascontiguousarray(v24.astype("<i4")[..., None].view(np.uint8)[..., :3]).reshape(T, 3 * C)
    forms["s24"] = (b24, v24.astype(np.float32) * np.float32(2.0 ** -23))
    s32 = g.integers(-2 ** 31, 2 ** 31, size=(T, C)).astype(np.int32)
    edge = (-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3)            # round to even: up and down
    s32.reshape(-1)[:min(4, T * C)] = edge[:min(4, T * C)]
    forms["s32"] = (s32, s32.astype(np.float32) * np.float32(2.0 ** -31))
    f32 = (0.3 * g.standard_normal((T, C))).astype(np.float32)
    forms["f32"] = (f32, f32)
    for name, table in (("ulaw", ulaw_table), ("alaw", alaw_table)):
        if T * C >= 256:
            codes = all_codes(T, C, seed=seed + len(name))
            assert len(np.unique(codes)) == 256
        else:
            codes = g.integers(0, 256, size=(T, C)).astype(np.uint8)
        forms[name] = (codes, table[codes].astype(np.float32) * np.float32(2.0 ** -15))
    return {k: (stored, np.ascontiguousarray(dec.T)) for k, (stored, dec) in forms.items()}


def chunkings(nbytes: int, rate: int, frame_bytes: int, history_bytes: int, slot_bytes: int):
    """name -> the chunk lengths (summing to nbytes) a feed loop is tried with: one byte at a time, a prime size (997 bytes),
    20 ms packets, 20 ms packets with an empty chunk among them, chunks shorter than the carried history, and one chunk
    larger than a slot (the whole recording when it is)"""
    def cut(size):
        return [min(size, nbytes - i) for i in range(0, nbytes, size)]
    packet = rate // 50 * frame_bytes
    with_empty = cut(packet)
    with_empty.insert(len(with_empty) // 2, 0)
    with_empty.insert(0, 0)
    big = max(2 * slot_bytes + frame_bytes + 1, nbytes // 2)
    out = {"bytes": [1] * nbytes, "prime": cut(997), "packets": cut(packet), "empty": with_empty,
           "short": cut(max(1, history_bytes // 3 + 1)), "big": [c for c in (min(big, nbytes), nbytes - min(big, nbytes)) if c]}
    assert all(sum(v) == nbytes for v in out.values())
    return out


def cut_bytes(data: bytes, sizes):
    """the chunks of `data` with the given lengths"""
    out, i = [], 0
    for k in sizes:
        out.append(data[i:i + k])
        i += k
    return out


def model_samples(bank64: np.ndarray, o: int, n: int, width: int, m0: int, m1: int, x: np.ndarray, first: int, total: int):
    """float64 [m1 - m0]: output samples m0 .. m1 of the polyphase filter, sample by sample, reading ONLY x = the decoded
    frames first .. first + len(x) of a recording of `total` frames (zero outside [0, total)); a tap that falls inside the
    recording but outside x is an error: the call would have read what it was not given.  bank64: [n, K] float64"""
    K = bank64.shape[1]
    j = np.arange(K)
    out = np.empty(m1 - m0, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    for m in range(m0, m1):
        f, p = divmod(m, n)
        idx = f * o + j - width
        inside = (idx >= 0) & (idx < total)
        rel = idx - first
        if not ((rel[inside] >= 0) & (rel[inside] < len(x))).all():
            raise IndexError(f"sample {m} reads frames outside the upload [{first}, {first + len(x)})")
        v = np.zeros(K, dtype=np.float64)
        v[inside] = x[rel[inside]]
        out[m - m0] = np.dot(bank64[p], v)
    return out
