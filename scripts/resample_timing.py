"""Where does a 48 kHz / 44.1 kHz recording spend its ingest time: the host resampler or the device one?

    python scripts/resample_timing.py [--minutes 30] [--out profiles/resample_timing.json]

Needs an MI355X (no fallback).  For each input rate a synthetic `--minutes` PCM16 mono WAV is written (the meeting-like signal of
testkit/synth.py at 16 kHz, brought to the rate with the host resampler and quantised), and these are recorded:

  * pipeline: `timings["load_s"]` / `["device_s"]` of DiariZenPipeline(resample="host") and (resample="device") on that file,
    the bench's model and batch (wavlm-large-s80, 8 s windows, batch 576, seeded weights), alternating the two modes after a
    warm-up call of each; host clock, each stage ends in a device-to-host copy.
  * kernel: device events around `--reps` launches of dzn_resample over the whole recording, its int16 frames already
    resident; bytes = the int16 input + the float32 output + the filter bank once, i.e. what the algorithm has to move.
  * host: audio.resample on the decoded float32 recording with the thread count this process is given (OMP_NUM_THREADS).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import struct
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def write_wav(path, pcm: np.ndarray, rate: int) -> None:
    body = pcm.astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, rate, 2 * rate, 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" +
                struct.pack("<I", len(body)))
        f.write(body)


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--rates", type=int, nargs="+", default=[48000, 44100])
    ap.add_argument("--reps", type=int, default=20, help="kernel launches in the timed window")
    ap.add_argument("--passes", type=int, default=3, help="timed pipeline calls per mode")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_timing.py measures on a HIP device; none is visible")
    from diarizen_amd import audio
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.synth import synth_recording_range
    from testkit.weights import emb_state_dict, turn_taking_state_dict

    dev = torch.device("cuda:0")
    cfg = get_seg_config("wavlm_large_s80_md")
    conf = {"model": {"path": "diarizen.models.eend.model_wavlm_conformer.Model",
                      "args": {"wavlm_src": "wavlm_large_s80_md", "wavlm_layer_num": cfg.wavlm_layer_num,
                               "wavlm_feat_dim": cfg.embed_dim, "chunk_size": 8}},
            "inference": {"args": {"seg_duration": 8, "segmentation_step": 0.1, "batch_size": 576,
                                   "apply_median_filtering": True}},
            "clustering": {"args": {"method": "AgglomerativeClustering", "min_speakers": 1, "max_speakers": 20,
                                    "ahc_criterion": "distance", "ahc_threshold": 0.1, "min_cluster_size": 13}}}
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(conf), device=dev, precision="f32h",
                            seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0))
    total16 = int(args.minutes * 60 * 16000)
    x16 = synth_recording_range(0, total16, total16).numpy()
    result = {"device": torch.cuda.get_device_name(0), "minutes": args.minutes, "host_threads": torch.get_num_threads(),
              "model": "wavlm_large_s80_md f32h, 8 s windows, batch 576, seeded weights", "rates": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for rate in args.rates:
            pcm = np.clip(np.rint(audio.resample(x16, 16000, rate) * 32768.0), -32768, 32767).astype(np.int16)
            path = os.path.join(tmp, f"synth_{rate}.wav")
            write_wav(path, pcm, rate)
            T = len(pcm)
            entry = {"input_samples": T}

            # ---- host resampler alone
            xf = pcm.astype(np.float32) * np.float32(1.0 / 32768.0)
            audio.resample(xf[:rate * 10], rate, 16000)                     # warm-up
            times = []
            for _ in range(3):
                t = time.perf_counter()
                y_host = audio.resample(xf, rate, 16000)
                times.append(time.perf_counter() - t)
            entry["host_resample_s"] = {"median": median(times), "all": times}

            # ---- kernel alone: the int16 frames resident, device events around `reps` launches
            bank, o, n, width = audio.resample_bank(rate, 16000)
            xd = torch.from_numpy(pcm).to(dev)
            y = audio.resample_device(xd, rate, 16000, device=dev)          # warm-up (uploads the bank, loads the code object)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                y = audio.resample_device(xd, rate, 16000, device=dev)
            e1.record()
            torch.cuda.synchronize()
            kernel_s = e0.elapsed_time(e1) * 1e-3 / args.reps
            alg_bytes = 2.0 * T + 4.0 * y.numel() + 4.0 * bank.size
            diff = np.abs(y.cpu().numpy().astype(np.float64) - y_host.astype(np.float64)).max()
            entry["kernel"] = {"seconds_per_launch": kernel_s, "launches": args.reps, "output_samples": int(y.numel()),
                               "taps": int(bank.shape[1]), "algorithmic_bytes": alg_bytes,
                               "achieved_bytes_per_s": alg_bytes / kernel_s,
                               "flop_per_s": 2.0 * y.numel() * bank.shape[1] / kernel_s,
                               "max_abs_diff_to_host_resampler": float(diff)}
            del xd, y

            # ---- the pipeline, both modes alternating
            modes = {"host": {"load_s": [], "device_s": []}, "device": {"load_s": [], "device_s": []}}
            for mode in modes:                                              # warm-up of both
                pipe.resample = mode
                pipe(path, sess_name="warmup")
            for _ in range(args.passes):
                for mode, rec in modes.items():
                    pipe.resample = mode
                    pipe(path, sess_name="timed")
                    rec["load_s"].append(pipe.timings["load_s"])
                    rec["device_s"].append(pipe.timings["device_s"])
            entry["pipeline"] = {mode: {"load_s": median(rec["load_s"]), "device_s": median(rec["device_s"]),
                                        "load_plus_device_s": median(np.add(rec["load_s"], rec["device_s"])), "all": rec}
                                 for mode, rec in modes.items()}
            result["rates"][str(rate)] = entry
            print(rate, json.dumps({k: v for k, v in entry.items() if k != "pipeline"}), flush=True)
            print(rate, json.dumps({m: {k: v for k, v in e.items() if k != "all"} for m, e in entry["pipeline"].items()}),
                  flush=True)
    pipe.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
