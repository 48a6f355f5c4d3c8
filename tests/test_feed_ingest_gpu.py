"""The stored-format mode of streaming.WaveIngest on the MI355X, with no model: 2 slots of 100 frames, so the ring wraps and
every slot is reused many times.  After every feed the final samples must be the schedule's (`ingest.n == feed_ready(frames)`)
and `dev_wave[:n]` the bits of `resample_device` of the WHOLE recording; after flush() the whole waveform, with zeros behind it.
Feeds at the model's rate go through dzn_decode and are compared with the host decode."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from testkit.feeds import SHAPES, chunkings, cut_bytes, stored_forms


def decode_choice(body: bytes, encoding: str, channels: int, channel):
    """float32 [frames]: the host decode of the channel choice (an index or "downmix") of whole stored frames"""
    from diarizen_amd.audio import _decode_frames
    return _decode_frames(body, encoding, channels, channel)


pytestmark = pytest.mark.gpu

WINDOW, STEP, SLOT_FRAMES, SLOTS = 640, 160, 100, 2
CHUNKINGS = ["bytes", "prime", "packets", "empty", "short", "big"]


def _feed_and_check(gpu, fmt, body: bytes, want: torch.Tensor, T: int):
    """every chunking of `body` (+ a partial frame) through a fresh WaveIngest; `want`: the whole-recording device result"""
    from diarizen_amd.audio import FeedPlanner, feed_ready, resampled_length
    from diarizen_amd.streaming import WaveIngest
    probe = FeedPlanner(fmt, 16000, SLOT_FRAMES)
    o, n, width, K = probe.o, probe.n, probe.width, probe.K
    M = resampled_length(T, o, n)
    assert want.shape == (M,)
    fb = fmt.frame_bytes
    data = body + b"\x5a" * (fb - 1)
    for name, sizes in chunkings(len(data), fmt.rate, fb, (K - 1) * fb, SLOT_FRAMES * fb).items():
        assert name in CHUNKINGS
        ing = WaveIngest(gpu, 16000, WINDOW, STEP, max_seconds=1.0, slots=SLOTS, feed_format=fmt, slot_frames=SLOT_FRAMES)
        assert len(ing.ring) == SLOTS and (ing.n, ing.frames) == (0, 0)
        bad = torch.zeros((), dtype=torch.int64, device=gpu)            # samples that differed after any feed (one sync)
        fed = 0
        for chunk in cut_bytes(data, sizes):
            before = ing.n
            made = ing.append(chunk)
            fed += len(chunk)
            assert ing.frames == fed // fb and made == ing.n - before
            assert ing.n == (ing.frames if probe.same_rate else feed_ready(ing.frames, o, n, width)), (name, fed)
            if made:
                ing.wait()
                bad += (ing.dev_wave[:ing.n] != want[:ing.n]).sum()
        assert ing.frames == T and ing.n < M or probe.same_rate
        ing.flush()
        assert ing.n == M and ing.flush() == 0 and ing.n == M
        ing.wait()
        assert int(bad) == 0, (name, "a prefix differed from the whole-recording result after some feed")
        assert torch.equal(ing.dev_wave[:M], want), name
        assert not ing.dev_wave[M:M + WINDOW].any(), name
        assert ing.uploads > SLOTS, "the ring wrapped"
        torch.cuda.synchronize()


@pytest.mark.parametrize("encoding", ["s16", "s24", "ulaw", "alaw", "f32"])
@pytest.mark.parametrize("rate,T,C", SHAPES)
def test_stored_feed_equals_the_whole_recording(built_lib, gpu, rate, T, C, encoding):
    from diarizen_amd.audio import FeedFormat, resample_device
    stored, _ = stored_forms(T, C, seed=rate + T)[encoding]
    channel = "downmix" if C == 3 else C - 1
    want = resample_device(stored, rate, 16000, device=gpu, channels=C, channel=channel, src_format=encoding)
    _feed_and_check(gpu, FeedFormat(rate, encoding, channels=C, channel=channel), stored.tobytes(), want, T)


@pytest.mark.parametrize("encoding,C,channel", [("s16", 2, "downmix"), ("s16", 2, 1), ("ulaw", 1, 0)])
def test_feed_at_the_model_rate_is_decoded(built_lib, gpu, encoding, C, channel):
    from diarizen_amd.audio import FeedFormat
    T = 1203
    stored, _ = stored_forms(T, C, seed=T + C)[encoding]
    want = torch.from_numpy(decode_choice(stored.tobytes(), encoding, C, channel)).to(gpu)
    _feed_and_check(gpu, FeedFormat(16000, encoding, channels=C, channel=channel), stored.tobytes(), want, T)


def test_refused_when_opened_and_capacity_counts_output_samples(built_lib, gpu):
    from diarizen_amd.audio import FeedFormat
    from diarizen_amd.streaming import WaveIngest
    with pytest.raises(ValueError, match="channel choice"):
        WaveIngest(gpu, 16000, WINDOW, STEP, max_seconds=1.0, feed_format=FeedFormat(8000, "ulaw", channels=2))
    with pytest.raises(ValueError, match="does not fit in LDS"):
        WaveIngest(gpu, 16000, WINDOW, STEP, max_seconds=1.0, feed_format=FeedFormat(15999, "s16", channel=0))
    ing = WaveIngest(gpu, 16000, WINDOW, STEP, max_seconds=0.1, feed_format=FeedFormat(8000, "ulaw", channel=0), slot_frames=SLOT_FRAMES)
    assert ing.append(bytes(800)) > 0                                   # 800 frames -> 1600 samples: max_seconds exactly
    with pytest.raises(MemoryError, match="max_seconds"):
        ing.append(bytes(1))
    ing.flush()
    assert ing.n == 1600
    torch.cuda.synchronize()
