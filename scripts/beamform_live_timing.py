"""What does the device ingest of a live ARRAY feed cost per slot, against a one-channel feed of the same format?

    python scripts/beamform_live_timing.py [--seconds 10] [--slots 6] [--out profiles/beamform_live_timing.json]

For 2, 8 and 64 channels of int16 at 16 kHz and 48 kHz a streaming.WaveIngest (16 kHz model rate) is fed `--slots` chunks of
`--seconds` each, one chunk per slot.  Device events on the ingest's copy stream bracket every append: the time is the upload of
the slot plus everything the planned call enqueues —

  * array:  FeedFormat(rate, "s16", channels=C, channel=Beamform(causal=True)): dzn_beamform_feed (planar decode, GCC-PHAT of
            the new blocks, the tracker, delay-and-sum) and, at 48 kHz, the carried history and dzn_resample;
  * mono:   FeedFormat(rate, "s16", channels=C, channel=0): dzn_decode / dzn_resample of one channel of the same frames —
            the path a user had to take before array feeds, which this feature does not touch.

append() first spends host time (planning, the copy of the slot into pinned memory) during which an idle stream would wait and
the span between the events would measure the host.  So before every append the copy stream is HELD by a spin kernel
(torch.cuda._sleep, `--hold-cycles`) and the first event is recorded behind it: the host work happens while the stream spins,
the enqueued work starts when the spin ends, and the span is device time alone.  `held_ms` is how long the stream was held;
the figures are valid when held_ms (the shortest hold) exceeds host_ms_max (the longest append).  The first slot
of a session (code objects, twiddles, banks) is reported apart; the figure is the median of the others.  Host time per append
is reported beside it.  Nothing here is a test and no test asserts a
time.  DESIGN.md §4.24 quotes the output.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def run(dev, fmt, chunks, seconds, hold_cycles):
    from diarizen_amd.streaming import WaveIngest
    ing = WaveIngest(dev, 16000, 128000, 12800, max_seconds=seconds * (len(chunks) + 1), slot_seconds=seconds, slots=4,
                     feed_format=fmt)
    events, host = [], []
    for ch in chunks:
        eh, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        eh.record(ing.copy_stream)
        with torch.cuda.stream(ing.copy_stream):
            torch.cuda._sleep(hold_cycles)
        e0.record(ing.copy_stream)
        t = time.perf_counter()
        ing.append(ch)
        host.append(1e3 * (time.perf_counter() - t))
        e1.record(ing.copy_stream)
        events.append((eh, e0, e1))
    ing.flush()
    ing.copy_stream.synchronize()
    ms = [b.elapsed_time(c) for _, b, c in events]
    held = [a.elapsed_time(b) for a, b, _ in events]
    return dict(first_ms=round(ms[0], 3), device_ms=round(statistics.median(ms[1:]), 3),
                device_ms_all=[round(v, 3) for v in ms[1:]], host_ms=round(statistics.median(host[1:]), 3),
                host_ms_max=round(max(host[1:]), 3), held_ms=round(min(held[1:]), 3), samples=int(ing.n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--slots", type=int, default=6)
    ap.add_argument("--hold-cycles", type=int, default=100_000_000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "beamform_live_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beamform_live_timing.py measures on a HIP device; none is visible")
    from diarizen_amd.audio import Beamform, FeedFormat
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    rows = []
    for rate in (16000, 48000):
        frames = int(a.seconds * rate)
        s = (3000.0 * g.standard_normal(frames * a.slots + 64)).astype(np.float32)
        for C in (2, 8, 64):
            x = np.stack([s[c % 32:c % 32 + frames * a.slots] for c in range(C)], axis=1)      # delayed copies, [N, C]
            x = x + 100.0 * g.standard_normal(x.shape).astype(np.float32)
            pcm = np.clip(np.rint(x), -32768, 32767).astype("<i2")
            chunks = [pcm[i * frames:(i + 1) * frames].tobytes() for i in range(a.slots)]
            bf = Beamform(causal=True)
            row = dict(rate=rate, channels=C, slot_seconds=a.seconds, slot_mb=round(len(chunks[0]) / 1e6, 2),
                       hop=bf.plan(rate, C)[0], max_lag=bf.plan(rate, C)[1],
                       array=run(dev, FeedFormat(rate, "s16", channels=C, channel=bf), chunks, a.seconds, a.hold_cycles),
                       mono=run(dev, FeedFormat(rate, "s16", channels=C, channel=0), chunks, a.seconds, a.hold_cycles))
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), slots=a.slots, rows=rows)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
