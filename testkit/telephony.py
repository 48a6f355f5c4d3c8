"""File writers for the telephony ingest tests (tests/test_telephony_host.py, tests/test_telephony_gpu.py): RIFF/WAVE and
NIST SPHERE files built by hand from their header layouts, so that the readers of diarizen_amd/audio.py are checked against
bytes they did not write.  Nothing under diarizen_amd/ imports this."""
from __future__ import annotations

import struct

import numpy as np

_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def wav_bytes(tag: int, channels: int, rate: int, bits: int, body: bytes, extensible: bool = False) -> bytes:
    """a RIFF/WAVE file: format `tag` (1 PCM, 3 float, 6 A-law, 7 mu-law), `bits` per sample, `body` = the interleaved
    frames; extensible: the tag goes into the SubFormat GUID of a WAVE_FORMAT_EXTENSIBLE fmt chunk"""
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, (1 << channels) - 1) + struct.pack("<H", tag) + _GUID_TAIL
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def sphere_bytes(coding, channels: int, rate: int, n_bytes: int, body: bytes, byte_format=None, header: int = 1024,
                 sample_count=None) -> bytes:
    """a NIST SPHERE file: `NIST_1A`, the header size, `name -type value` lines, `end_head`, padding to `header` bytes, then
    `body` = the interleaved frames.  coding None: no sample_coding field (pcm); sample_count None: what `body` holds"""
    if sample_count is None:
        sample_count = len(body) // (channels * n_bytes)
    if byte_format is None:
        byte_format = "1" if n_bytes == 1 else "01"
    fields = [("database_id", "-s8", "testfile"), ("channel_count", "-i", channels), ("sample_count", "-i", sample_count),
              ("sample_rate", "-i", rate), ("sample_n_bytes", "-i", n_bytes),
              ("sample_byte_format", f"-s{len(byte_format)}", byte_format), ("sample_sig_bits", "-i", 8 * n_bytes)]
    if coding is not None:
        fields.append(("sample_coding", f"-s{len(coding)}", coding))
    text = "NIST_1A\n%7d\n" % header + "".join(f"{k} {t} {v}\n" for k, t, v in fields) + "end_head\n"
    head = text.encode("ascii")
    assert len(head) <= header
    return head + b" " * (header - len(head)) + body


def all_codes(frames: int, channels: int, seed: int) -> np.ndarray:
    """uint8 [frames, channels] of seeded G.711 code bytes in which every one of the 256 codes occurs"""
    assert frames * channels >= 256
    x = np.random.default_rng(seed).integers(0, 256, size=frames * channels).astype(np.uint8)
    x[:256] = np.arange(256, dtype=np.uint8)
    return np.random.default_rng(seed + 1).permutation(x).reshape(frames, channels)
