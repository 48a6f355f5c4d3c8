"""Shared by test_detection_stream_gpu.py and test_live_diarization_gpu.py: the recordings cut from the 30 s fixture, the window
geometry they are named after, and the chunking of a feed loop.  numpy and the package's audio reader only; nothing here touches
a device."""
from __future__ import annotations

import io
import os
import wave as _wave

WAV = os.path.join(os.path.dirname(__file__), "golden", "EN2002a_30s.wav")
WINDOW, STEP, FEED = 128000, 12800, 5920            # 8 s windows at a 0.8 s step; 0.37 s per feed
RECORDINGS = {"grid": WINDOW + 10 * STEP,           # 16 s: the last window ends with the recording, no padded window
              "padded": 480000,                     # 30 s: 28 windows and a zero-padded 29th
              "short": 80000}                       # 5 s: one zero-padded window, nothing is committed before finish()


def samples(n):
    """the first n samples of the fixture: (float32 array, in-memory 16-bit WAV)"""
    from diarizen_amd.audio import first_channel_16k
    with _wave.open(WAV, "rb") as r:
        assert r.getframerate() == 16000 and r.getnchannels() == 1 and r.getsampwidth() == 2 and r.getnframes() >= n
        pcm = r.readframes(n)
    buf = io.BytesIO()
    with _wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm)
    x = first_channel_16k(buf.getvalue())
    assert len(x) == n
    return x, buf.getvalue()


def feeds(x, size=FEED):
    return [x[i:i + size] for i in range(0, len(x), size)]
