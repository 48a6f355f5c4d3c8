"""What does a two-channel 8 kHz mu-law call cost to bring onto the device at 16 kHz: host decode + host resampler + float32
upload, or the stored bytes uploaded and decoded by the device resampler?

    python scripts/telephony_timing.py [--minutes 30] [--runs 7] [--out profiles/telephony_timing.json]

Needs an MI355X (no fallback).  A synthetic `--minutes` recording (testkit/synth.py at 16 kHz, brought to 8 kHz with the host
resampler; channel 1 is channel 0 delayed by 0.5 s) is written as a mu-law WAV and as the same payload in SPHERE.  For every
file, channel choice and `resample=` mode the wall time of `open_recording` + `recording_on_device` is taken after one warm-up
call, the clock stopped after `torch.cuda.synchronize()`; the median of `--runs` calls and the bytes uploaded are recorded."""
from __future__ import annotations

import argparse
import audioop
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "telephony_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("telephony_timing.py measures on a HIP device; none is visible")
    from diarizen_amd import audio
    from diarizen_amd.pipeline import open_recording, recording_on_device
    from testkit.synth import synth_recording_range
    from testkit.telephony import sphere_bytes, wav_bytes

    dev = torch.device("cuda:0")
    total16 = int(args.minutes * 60 * 16000)
    x8 = audio.resample(synth_recording_range(0, total16, total16).numpy(), 16000, 8000)
    x = np.stack([x8, np.concatenate([np.zeros(4000, dtype=np.float32), x8[:-4000]])], axis=1)
    pcm = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    codes = audioop.lin2ulaw(pcm.tobytes(), 2)
    frames = len(pcm)
    result = {"device": torch.cuda.get_device_name(0), "minutes": args.minutes, "host_threads": torch.get_num_threads(),
              "runs": args.runs, "frames_8k": frames, "file_bytes": len(codes), "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        files = {"wav": os.path.join(tmp, "call.wav"), "sphere": os.path.join(tmp, "call.sph")}
        Path(files["wav"]).write_bytes(wav_bytes(7, 2, 8000, 8, codes))
        Path(files["sphere"]).write_bytes(sphere_bytes("ulaw", 2, 8000, 1, codes))
        for kind, path in files.items():
            for channel in (0, "downmix"):
                for mode in ("host", "device"):
                    times = []
                    for i in range(args.runs + 1):                          # the first call is the warm-up
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        wave = recording_on_device(open_recording(path, 16000, resample=mode, device=dev, channel=channel), dev)
                        torch.cuda.synchronize()
                        if i:
                            times.append(time.perf_counter() - t)
                    assert wave.shape == (2 * frames,) and wave.dtype == torch.float32
                    # host: the float32 waveform at 16 kHz; device: the stored frames, both channels, one byte per sample
                    uploaded = 4 * 2 * frames if mode == "host" else 2 * frames
                    case = {"file": kind, "channel": channel, "resample": mode, "median_s": float(np.median(times)),
                            "all_s": times, "bytes_uploaded": uploaded}
                    result["cases"].append(case)
                    print(json.dumps({k: v for k, v in case.items() if k != "all_s"}), flush=True)
                    del wave
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
