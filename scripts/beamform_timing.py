"""What does GCC-PHAT delay-and-sum beamforming of an array recording cost, against the device stage it feeds?

    python scripts/beamform_timing.py [--minutes 30] [--channels 8] [--out profiles/beamform_timing.json]

Needs an MI355X (no fallback).  A synthetic `--minutes`, `--channels`-channel, 16 kHz int16 WAV is written: the meeting-like
signal of testkit/synth.py, delayed per channel by up to +-40 samples, plus independent noise.  Recorded:

  * kernels: device events around `--reps` whole-recording launches of dzn_beamform_delays and of dzn_beamform_sum, the planar
    float32 channels already resident (what the two kernels cost without the file, the upload and the decode).
  * source: host clock around BeamformedSource.read_device(0, T) of the file — read, upload as stored, dzn_decode per channel,
    delays, smoothing on the host, sum — ending in a device synchronise; the first read (estimates the delays) and later ones.
  * pipeline: `timings["load_s"]` / `["device_s"]` of DiariZenPipeline on that file with channel=0 and with
    channel=Beamform(), the bench's model and batch, alternating after a warm-up call of each.  device_s of the Beamform run
    contains the beamforming (the source makes its samples inside device_stage).
  * numpy: the float32 restatement (testkit/beamform_ref.py: raw_delays) on `--numpy-blocks` blocks, as milliseconds per
    (block, channel pair) on this host.
"""
from __future__ import annotations

import argparse
import copy
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


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5, help="kernel launches in the timed window")
    ap.add_argument("--passes", type=int, default=3, help="timed pipeline calls per channel choice")
    ap.add_argument("--numpy-blocks", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "beamform_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beamform_timing.py measures on a HIP device; none is visible")
    from diarizen_amd import audio
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline, open_recording
    from testkit import beamform_ref
    from testkit.synth import synth_recording_range
    from testkit.telephony import wav_bytes
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
    T, C = int(args.minutes * 60 * 16000), args.channels
    s = synth_recording_range(0, T, T).numpy()
    g = np.random.default_rng(7)
    true = [0] + [int(d) for d in g.integers(-40, 41, size=C - 1)]
    pcm = np.empty((T, C), dtype="<i2")
    for c, d in enumerate(true):
        xc = beamform_ref.delayed_copies(s, (d,), 0.0, 0)[0] + (0.01 * g.standard_normal(T)).astype(np.float32)
        pcm[:, c] = np.clip(np.rint(xc * 32768.0), -32768, 32767)
    del s, xc
    bf = audio.Beamform()
    hop, max_lag, min_peak = bf.plan(16000, C)
    nb = audio.beamform_blocks(T, hop)
    result = {"device": torch.cuda.get_device_name(0), "minutes": args.minutes, "channels": C, "samples": T, "hop": hop,
              "max_lag": max_lag, "blocks": nb, "block_channel_pairs": nb * (C - 1), "true_delays": true,
              "model": "wavlm_large_s80_md f32h, 8 s windows, batch 576, seeded weights"}

    # ---- numpy restatement on a short stretch
    k = args.numpy_blocks
    xs = np.ascontiguousarray(pcm[:(k - 1) * hop].T.astype(np.float32) / 32768.0)
    beamform_ref.raw_delays(xs[:, :4 * hop], 0, hop, max_lag, np.float32)
    t = time.perf_counter()
    beamform_ref.raw_delays(xs, 0, hop, max_lag, np.float32)
    result["numpy_float32_ms_per_block_pair"] = (time.perf_counter() - t) * 1e3 / (k * (C - 1))

    # ---- the two kernels alone, planar float32 resident
    planar = torch.from_numpy(np.ascontiguousarray(pcm.T)).to(dev).to(torch.float32).mul_(1.0 / 32768.0)
    kw = dict(device=dev, reference=0, hop=hop, max_lag=max_lag)
    lag, peak = audio.beamform_delays_device(planar, **kw)              # warm-up (uploads the twiddles, loads the code object)
    delays = audio.smooth_delays(lag.cpu().numpy(), peak.cpu().numpy(), T, hop, min_peak)
    result["delays_recovered"] = bool((delays == np.array(true)[:, None]).all())
    d_delays = torch.from_numpy(delays).to(dev)
    y = audio.beamform_sum_device(planar, d_delays, device=dev, hop=hop)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    for _ in range(args.reps):
        audio.beamform_delays_device(planar, **kw)
    e[1].record()
    for _ in range(args.reps):
        audio.beamform_sum_device(planar, d_delays, device=dev, hop=hop, out=y)
    e[2].record()
    torch.cuda.synchronize()
    delays_s, sum_s = e[0].elapsed_time(e[1]) * 1e-3 / args.reps, e[1].elapsed_time(e[2]) * 1e-3 / args.reps
    ffts = nb * (2 * C - 1)
    W = 2 * hop
    result["kernels"] = {"delays_s": delays_s, "sum_s": sum_s, "launches": args.reps, "transforms": ffts,
                         "us_per_block_pair": delays_s * 1e6 / (nb * (C - 1)),
                         "transform_flop_per_s": ffts * 5.0 * W * np.log2(W) / delays_s,
                         "sum_bytes_per_s": 4.0 * T * (C + 1) / sum_s}
    del planar, y, lag, peak
    torch.cuda.empty_cache()

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "array.wav")
        with open(path, "wb") as f:
            f.write(wav_bytes(1, C, 16000, 16, pcm.tobytes()))
        del pcm

        # ---- the source on its own
        reads = []
        for i in range(3):
            src = open_recording(path, 16000, device=dev, channel=bf)
            for which in ("first_read_s", "second_read_s"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                src.read_device(0, T)
                torch.cuda.synchronize()
                reads.append((which, time.perf_counter() - t))
        result["source"] = {w: median([v for n, v in reads[2:] if n == w]) for w in ("first_read_s", "second_read_s")}
        result["source"]["all"] = reads

        # ---- the pipeline, both channel choices alternating
        modes = {"channel_0": (0, {"load_s": [], "device_s": []}), "beamform": (bf, {"load_s": [], "device_s": []})}
        for choice, _ in modes.values():
            pipe.channel = choice
            pipe(path, sess_name="warmup")
        for _ in range(args.passes):
            for choice, rec in modes.values():
                pipe.channel = choice
                pipe(path, sess_name="timed")
                rec["load_s"].append(pipe.timings["load_s"])
                rec["device_s"].append(pipe.timings["device_s"])
        result["pipeline"] = {name: {"load_s": median(rec["load_s"]), "device_s": median(rec["device_s"]),
                                     "load_plus_device_s": median(np.add(rec["load_s"], rec["device_s"])), "all": rec}
                              for name, (_, rec) in modes.items()}
    pipe.close()
    print(json.dumps({k: v for k, v in result.items() if k not in ("source", "pipeline")}), flush=True)
    print(json.dumps({k: v for k, v in result["source"].items() if k != "all"}), flush=True)
    print(json.dumps({m: {k: v for k, v in r.items() if k != "all"} for m, r in result["pipeline"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
