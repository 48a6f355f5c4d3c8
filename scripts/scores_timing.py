"""What per-speaker activity scores cost on the bench's 30-min workload, in one process on one device: wavlm-large-s80, 8 s
windows at a 0.8 s step (2241 windows), seeded turn-taking weights, the synthetic recording of bench.py (seed 3407) as an
in-memory 16-bit WAV, batch 576.  `pipeline(wav)` and `pipeline(wav, return_scores=True)` are each timed over `--steps` calls
after one untimed call; the device stage and the host stage are the pipeline's own `timings`.  Then the two new passes on
their own: the classifier launch with and without the soft output (the engine's per-kernel profile of one batch) and
dzn_speaker_scores alone on the recording's soft scores and clusters (HIP events around the call).

    timeout -k 10 900 python scripts/scores_timing.py            # -> profiles/scores_timing_30min_b576.json
    ... --bench-parent A.json B.json --bench-this C.json D.json   # also record four plain `python bench.py` result lines
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

from detect_timing import wav_blob  # noqa: E402


def scores_kernel_ms(soft: torch.Tensor, hard: np.ndarray, chunks, reps: int = 20):
    """median time of one dzn_speaker_scores call on device soft scores [C, L, S]"""
    from diarizen_amd import _lib
    from diarizen_amd.postprocess import _frame_grid, aggregation_windows, receptive_field
    lib = _lib.load()
    Cn, L, S = soft.shape
    _, starts, T = _frame_grid(Cn, L, chunks, receptive_field())
    K = int(hard.max()) + 1
    dev = soft.device
    d_start = torch.from_numpy(starts).to(dev)
    d_hard = torch.from_numpy(np.ascontiguousarray(hard, dtype=np.int8)).to(dev)
    d_ham, d_wu = (torch.from_numpy(w).to(dev) for w in aggregation_windows(L, chunks.duration))
    sc = torch.empty((T, K), device=dev, dtype=torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    st = torch.cuda.current_stream(dev)
    times = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        _lib.check(lib.dzn_speaker_scores(p(soft), p(d_hard), Cn, L, S, p(d_start), p(d_ham), p(d_wu), T, K, p(sc),
                                          C.c_void_p(st.cuda_stream)), None, "dzn_speaker_scores")
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"windows": Cn, "frames": T, "clusters": K, "ms_median": round(float(np.median(times[2:])), 4),
            "ms_min": round(float(np.min(times[2:])), 4), "reps": reps}


def classify_ms(engine, chunk: torch.Tensor, reps: int = 5):
    """the classifier launch of one batch with and without the soft output: the engine's per-kernel profile"""
    from diarizen_amd import _lib
    out = {"windows": int(chunk.shape[0])}
    for key, soft in (("logp_and_decisions", False), ("with_soft", True)):
        engine.segment(chunk, want_logp=False, want_soft=soft)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_collect()
        for _ in range(reps):
            engine.segment(chunk, want_logp=False, want_soft=soft)
        torch.cuda.synchronize()
        prof = {e["name"]: e for e in _lib.profile_collect()}
        _lib.profile_enable(False)
        e = prof.get("classify")
        out[key + "_ms"] = round(e["ms"] / max(e["launches"], 1), 4) if e else None
    return out


def last_json_line(path: str):
    lines = [ln for ln in Path(path).read_text().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=576)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files holding a plain bench.py result line of the parent commit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="files holding a plain bench.py result line of this commit")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "scores_timing_30min_b576.json"))
    a = ap.parse_args()
    from diarizen_amd.clustering import active_speakers
    from diarizen_amd.configs import get_seg_config
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
    res = {"workload": f"{a.minutes:g} min synthetic recording (seed 3407), wavlm_large_s80_md, 8 s windows, step 0.8 s, "
                       f"batch {a.batch}, seeded turn-taking weights, in-memory 16-bit WAV",
           "device": torch.cuda.get_device_name(dev), "steps": a.steps, "audio_s": audio_s}
    runs = {"pipeline": lambda: pipe(blob, "bench"), "pipeline_return_scores": lambda: pipe(blob, "bench", return_scores=True)}
    rttm = {}
    for name, fn in runs.items():
        fn()                                   # untimed: tables, allocator, the second engine handle
        per = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            out = fn()
            torch.cuda.synchronize()
            per.append(dict(pipe.timings))
        ann = out[0] if isinstance(out, tuple) else out
        rttm[name] = ann.to_rttm()
        res[name] = {k: [round(t[k], 4) for t in per] for k in ("load_s", "device_s", "host_s")}
        res[name]["audio_seconds_per_s"] = round(audio_s / float(np.mean([t["load_s"] + t["device_s"] + t["host_s"] for t in per])), 1)
        if isinstance(out, tuple):
            res[name]["scores_shape"] = list(out[1].data.shape)
        print(name, res[name], flush=True)
    res["same_rttm"] = rttm["pipeline"] == rttm["pipeline_return_scores"]
    res["engine_handles"] = 1 + len(pipe.extra_engines)
    # the two new passes alone
    wave = torch.from_numpy(x).to(dev)
    r = pipe._runner
    views = r.windows_view(wave)
    res["classify_kernel"] = classify_ms(pipe.engine, views[:min(a.batch, views.shape[0])].contiguous())
    seen = {}
    inner = pipe.clustering

    def spy(**kw):
        o = inner(**kw)
        seen["hard"], seen["seg"] = np.array(o[0], copy=True), kw["segmentations"]
        return o
    pipe.clustering = spy
    pipe(blob, "bench")
    pipe.clustering = inner
    hard = seen["hard"]
    hard[~active_speakers(seen["seg"])] = -2
    soft = r.run(wave, with_embeddings=False, with_scores=True).scores
    res["dzn_speaker_scores_30min"] = scores_kernel_ms(soft, hard, pipe.chunks_window())
    print("classify", res["classify_kernel"], "dzn_speaker_scores", res["dzn_speaker_scores_30min"], flush=True)
    pipe.close()
    if a.bench_parent or a.bench_this:
        keep = ("value", "unit", "steps", "warmup", "step_s", "commit")
        rows = {"parent": [last_json_line(f) for f in a.bench_parent], "this": [last_json_line(f) for f in a.bench_this]}
        res["plain_bench"] = {k: [{kk: row[kk] for kk in keep if kk in row} or row for row in v] for k, v in rows.items()}
        for k, v in rows.items():
            vals = [row.get("value") for row in v if isinstance(row.get("value"), (int, float))]
            if vals:
                res["plain_bench"][k + "_mean"] = round(float(np.mean(vals)), 2)
                res["plain_bench"][k + "_spread"] = round(float(max(vals) - min(vals)), 2)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("pipeline", "pipeline_return_scores", "same_rttm")}))


if __name__ == "__main__":
    main()
