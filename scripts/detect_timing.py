"""Voice activity / overlapped speech detection beside DiariZenPipeline on the bench's 30-min workload, in one process on one
device: wavlm-large-s80, 8 s windows at a 0.8 s step (2241 windows), seeded turn-taking weights, the synthetic recording of
bench.py (seed 3407) as an in-memory 16-bit WAV, batch 576.  Each pipeline is timed over `--steps` calls after one untimed
call (decode + upload + device stage + host stage + RTTM text each).  The detection pipelines are built from the diarization
pipeline, i.e. they run on its engine handle(s) and skip the embedding model and the clustering.  Then dzn_detect alone
(both tasks, aggregation + hysteresis) on the 30-min decisions and on a 4 h decision array, HIP events around the call.

    timeout -k 10 900 python scripts/detect_timing.py            # -> profiles/detect_timing_30min_b576.json
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import io
import json
import sys
import time
import wave as _wave
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def wav_blob(x: np.ndarray) -> bytes:
    buf = io.BytesIO()
    with _wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes((np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
    return buf.getvalue()


def kernel_ms(seg: torch.Tensor, chunks, reps: int = 20):
    """median time of one dzn_detect call (tasks = speech | overlap) on device decisions [C, L, S]"""
    from diarizen_amd import _lib
    from diarizen_amd.postprocess import _frame_grid, detection_weights, receptive_field
    lib = _lib.load()
    Cn, L, S = seg.shape
    _, starts, T = _frame_grid(Cn, L, chunks, receptive_field())
    dev = seg.device
    d_start = torch.from_numpy(starts).to(dev)
    d_w = torch.from_numpy(detection_weights(L, chunks.duration)).to(dev)
    sc = torch.empty((T, 2), device=dev, dtype=torch.float32)
    act = torch.empty((T, 2), device=dev, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = torch.cuda.current_stream(dev)
    times = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        _lib.check(lib.dzn_detect(p(seg), Cn, L, S, p(d_start), p(d_w), T, 3, 0.5, 0.5, p(sc), p(act),
                                  C.c_void_p(st.cuda_stream)), None, "dzn_detect")
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"windows": Cn, "frames": T, "ms_median": round(float(np.median(times[2:])), 4),
            "ms_min": round(float(np.min(times[2:])), 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=576)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "detect_timing_30min_b576.json"))
    a = ap.parse_args()
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.detection import OverlappedSpeechDetection, VoiceActivityDetection
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.synth import synth_recording
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    dev = torch.device("cuda:0")
    cfg = get_seg_config("wavlm_large_s80_md")
    conf = {"model": {"path": "diarizen.models.eend.model_wavlm_conformer.Model",
                      "args": {"wavlm_src": "wavlm_large_s80_md", "wavlm_layer_num": cfg.wavlm_layer_num,
                               "wavlm_feat_dim": cfg.embed_dim, "chunk_size": 8}},
            "inference": {"args": {"seg_duration": 8, "segmentation_step": 0.1, "batch_size": a.batch,
                                   "apply_median_filtering": True}},
            "clustering": {"args": {"method": "AgglomerativeClustering", "min_speakers": 1, "max_speakers": 20,
                                    "ahc_criterion": "distance", "ahc_threshold": 0.1, "min_cluster_size": 13}}}
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(conf), device=dev, seg_state=turn_taking_state_dict(cfg, 0),
                            emb_state=emb_state_dict(0))
    x = synth_recording(int(a.minutes * 60 * 16000)).numpy()
    blob = wav_blob(x)
    audio_s = len(x) / 16000.0
    pipe(blob, "bench")                        # untimed: tables, allocator, the second engine handle
    vad, osd = VoiceActivityDetection(pipe), OverlappedSpeechDetection(pipe)
    res = {"workload": f"{a.minutes:g} min synthetic recording (seed 3407), wavlm_large_s80_md, 8 s windows, step 0.8 s, "
                       f"batch {a.batch}, seeded turn-taking weights, in-memory 16-bit WAV",
           "device": torch.cuda.get_device_name(dev), "steps": a.steps, "audio_s": audio_s}
    runs = {"diarization": lambda: pipe(blob, "bench"), "vad": lambda: vad({"audio": blob, "uri": "bench"}),
            "osd": lambda: osd({"audio": blob, "uri": "bench"})}
    for name in ("vad", "osd"):
        runs[name]()                           # untimed
    for name, fn in runs.items():
        per = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t0)
        res[name] = {"audio_seconds_per_s": round(audio_s / float(np.mean(per)), 1), "s_per_call": [round(t, 4) for t in per],
                     "regions": len(list(out.itertracks()))}
        print(name, res[name], flush=True)
    res["engine_handles"] = 1 + len(pipe.extra_engines)
    # dzn_detect alone: the 30-min decisions of this recording (raw, median filter off) and a 4 h decision array
    r = vad._runner.run(torch.from_numpy(x).to(dev), with_embeddings=False)
    chunks = SlidingWindow(start=0.0, duration=8.0, step=0.1 * 8.0)
    res["dzn_detect_30min"] = kernel_ms(r.segmentations, chunks)
    g = np.random.default_rng(7)
    tog = g.random((17991, 399, 4), dtype=np.float32) < 0.03
    seg4 = torch.from_numpy((np.cumsum(tog, axis=1) % 2).astype(np.uint8)).to(dev)
    res["dzn_detect_4h"] = kernel_ms(seg4, chunks)
    print("dzn_detect", res["dzn_detect_30min"], res["dzn_detect_4h"], flush=True)
    pipe.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("diarization", "vad", "osd")}))


if __name__ == "__main__":
    main()
