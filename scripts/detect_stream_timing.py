"""What one feed of a detection stream (diarizen_amd/detection.py, DetectionStream) costs on the device once a new window is
complete, against what it replaces: on the 30-min workload of scripts/detect_timing.py (wavlm-large-s80, 8 s windows at a 0.8 s
step, 2241 windows, seeded turn-taking weights, the synthetic recording of bench.py, raw decisions with the median filter off)

  * dzn_detect_range over [start frame of the newest window, frames covered): the frames that window changed, hysteresis
    entered with the committed state — after window 1120 (mid-recording) and after window 2240 (the last one);
  * dzn_detect over all frames of the windows so far, which is what a stream without the range form would run per feed.

Both tasks per call (speech | overlap), HIP events around the call, median and minimum over `--reps` calls after two untimed.

    timeout -k 10 600 python scripts/detect_stream_timing.py        # -> profiles/detect_stream_timing_30min.json
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, st, reps):
    times = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(float(np.median(times[2:])), 4), "ms_min": round(float(np.min(times[2:])), 4), "reps": reps}


def feed_ms(seg: torch.Tensor, chunks, upto: int, reps: int):
    """windows 0 .. upto - 1 are complete, the last of them is new: the range call of that feed and the whole-recording call"""
    from diarizen_amd import _lib
    from diarizen_amd.postprocess import _frame_grid, committed_frames, detect_range_launch, detection_weights, receptive_field
    lib = _lib.load()
    _, L, S = seg.shape
    frames = receptive_field()
    _, starts, T = _frame_grid(upto, L, chunks, frames)
    dev = seg.device
    d_start = torch.from_numpy(starts).to(dev)
    d_w = torch.from_numpy(detection_weights(L, chunks.duration)).to(dev)
    sc = torch.empty((T, 2), device=dev, dtype=torch.float32)
    act = torch.empty((T, 2), device=dev, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = torch.cuda.current_stream(dev)

    def whole():
        _lib.check(lib.dzn_detect(p(seg), upto, L, S, p(d_start), p(d_w), T, 3, 0.5, 0.5, p(sc), p(act),
                                  C.c_void_p(st.cuda_stream)), None, "dzn_detect")
    res = {"windows": upto, "frames": T, "dzn_detect": timed(whole, st, reps)}
    t0 = committed_frames(upto - 1, chunks, frames)          # the frontier before the newest window arrived
    entry = act[t0 - 1].clone() if t0 > 0 else None
    sc_r = torch.empty((T - t0, 2), device=dev, dtype=torch.float32)
    act_r = torch.empty((T - t0, 2), device=dev, dtype=torch.uint8)

    def ranged():
        _lib.check(lib.dzn_detect_range(p(seg), upto, L, S, p(d_start), p(d_w), t0, T, 3, 0.5, 0.5,
                                        p(entry) if entry is not None else None, p(sc_r), p(act_r),
                                        C.c_void_p(st.cuda_stream)), None, "dzn_detect_range")
    res["dzn_detect_range"] = dict(timed(ranged, st, reps), t0=t0, t1=T, frames=T - t0)
    torch.cuda.synchronize()
    assert torch.equal(act_r, act[t0:]) and torch.equal(sc_r.view(torch.int32), sc[t0:].view(torch.int32))
    # the wrapper the stream uses (allocates its two outputs per call)
    res["detect_range_launch"] = timed(lambda: detect_range_launch(seg, upto, d_start, d_w, t0, T, 3, 0.5, 0.5, entry), st, reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=576)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "detect_stream_timing_30min.json"))
    a = ap.parse_args()
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.detection import VoiceActivityDetection
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
    vad = VoiceActivityDetection(pipe)
    x = synth_recording(int(a.minutes * 60 * 16000)).numpy()
    seg = vad._runner.run(torch.from_numpy(x).to(dev), with_embeddings=False).segmentations
    torch.cuda.synchronize()
    chunks = SlidingWindow(start=0.0, duration=8.0, step=0.1 * 8.0)
    Cn = seg.shape[0]
    res = {"workload": f"{a.minutes:g} min synthetic recording (seed 3407), wavlm_large_s80_md, 8 s windows, step 0.8 s, "
                       f"{Cn} windows, seeded turn-taking weights, raw decisions; tasks = speech | overlap",
           "device": torch.cuda.get_device_name(dev),
           "after_last_window": feed_ms(seg, chunks, Cn, a.reps),
           "after_middle_window": feed_ms(seg, chunks, (Cn + 1) // 2, a.reps)}
    pipe.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
