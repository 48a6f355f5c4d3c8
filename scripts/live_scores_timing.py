"""What live per-speaker activity scores cost, on one device: wavlm-large-s80, 8 s windows at a 0.8 s step, seeded turn-taking
weights, the synthetic recording of bench.py (seed 3407).

  solo   one `open_live` session fed 0.8 s per feed, so that every timed feed completes exactly one window: upload, one
         forward of one window, the host labelling, ONE range launch, the D2H of its rows.
  hub    16 sessions in one `open_hub`, each fed 0.8 s per round, one tick() per round: one upload, one ingest launch, one
         forward of 16 windows, 16 range launches.

The time of a feed / tick is a host clock between two device synchronisations (the step itself ends in the D2H of the new
rows).  Every measurement is a process of its own (`--child`); the driver runs them one after the other and alternates
[this tree without scores, the parent tree without scores, this tree with scores] `--rounds` times, so that the three share the
box's state.  The parent tree is a checkout of the parent commit with its own built library (`--parent-root`); without it only
this tree is measured.

    timeout -k 10 900 python scripts/live_scores_timing.py --parent-root <checkout of the parent commit>
        -> profiles/live_scores_timing.json
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
STEP, WINDOW = 12800, 128000


def child(a) -> None:
    root = Path(a.root).resolve()
    sys.path.insert(0, str(root))
    import numpy as np
    import torch
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.synth import synth_recording
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    import diarizen_amd
    assert Path(diarizen_amd.__file__).resolve().parents[1] == root, "the package was not imported from --root"
    dev = torch.device("cuda:0")
    cfg = get_seg_config("wavlm_large_s80_md")
    conf = {"model": {"path": "diarizen.models.eend.model_wavlm_conformer.Model",
                      "args": {"wavlm_src": "wavlm_large_s80_md", "wavlm_layer_num": cfg.wavlm_layer_num,
                               "wavlm_feat_dim": cfg.embed_dim, "chunk_size": 8}},
            "inference": {"args": {"seg_duration": 8, "segmentation_step": 0.1, "batch_size": 64,
                                   "apply_median_filtering": True}},
            "clustering": {"args": {"method": "AgglomerativeClustering", "min_speakers": 1, "max_speakers": 20,
                                    "ahc_criterion": "distance", "ahc_threshold": 0.1, "min_cluster_size": 13}}}
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(conf), device=dev, seg_state=turn_taking_state_dict(cfg, 0),
                            emb_state=emb_state_dict(0))
    kw = {"scores": True} if a.scores else {}                       # (the parent tree has no such keyword)
    x = synth_recording(int(a.seconds * 16000)).numpy()
    chunks = [x[i:i + STEP] for i in range(0, len(x) - STEP + 1, STEP)]
    times = []

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    if a.mode == "solo":
        for rep in range(2):                                        # the first session warms tables, allocator and code objects
            sess = pipe.open_live(sess_name="s", delta_new=0.2, max_seconds=a.seconds + 10, **kw)
            for i, c in enumerate(chunks):
                ms = timed(lambda: sess.feed(c))
                if rep and (i + 1) * STEP >= WINDOW + STEP:          # feeds that complete exactly one window, the first one left out
                    times.append(ms)
            windows, calls = sess.done, sess.stats["range_calls"]
            sess.finish()
        extra = {"windows": windows, "range_calls": calls}
    else:
        for rep in range(2):
            with pipe.open_hub(max_sessions=a.sessions, max_seconds=a.seconds + 10) as hub:
                ss = [hub.open(f"s{j}", delta_new=0.2, **kw) for j in range(a.sessions)]
                for i, c in enumerate(chunks):
                    for j, s in enumerate(ss):
                        s.feed(np.roll(c, 37 * j))
                    ms = timed(hub.tick)
                    if rep and (i + 1) * STEP >= WINDOW + STEP:
                        times.append(ms)
                extra = {"sessions": a.sessions, "forwards": hub.stats["total"]["forwards"],
                         "range_calls": hub.stats["total"]["range_calls"], "windows": hub.stats["total"]["windows"]}
    pipe.close()
    t = np.array(times)
    print(json.dumps(dict(extra, mode=a.mode, scores=bool(a.scores), n=len(t), ms_median=round(float(np.median(t)), 4),
                          ms_p10=round(float(np.percentile(t, 10)), 4), ms_p90=round(float(np.percentile(t, 90)), 4),
                          ms_min=round(float(t.min()), 4), device=torch.cuda.get_device_name(dev))))


def run_child(root: Path, mode: str, scores: bool, a) -> dict:
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--root", str(root), "--mode", mode, "--seconds", str(a.seconds),
           "--sessions", str(a.sessions)] + (["--scores"] if scores else [])
    env = dict(os.environ, PYTHONPATH=str(root))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout, env=env, cwd=str(root))
    if r.returncode != 0:                                            # a failed measurement ends the run: nothing more starts on the device
        raise SystemExit(f"child {cmd} failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def summary(rows: list) -> dict:
    med = [r["ms_median"] for r in rows]
    return {"runs_ms_median": med, "mean_of_medians_ms": round(sum(med) / len(med), 4), "spread_ms": round(max(med) - min(med), 4),
            "runs_ms_p10_p90": [[r["ms_p10"], r["ms_p90"]] for r in rows], "n_per_run": rows[0]["n"],
            **{k: rows[0][k] for k in ("windows", "range_calls", "forwards", "sessions") if k in rows[0]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--mode", choices=("solo", "hub"), default="solo")
    ap.add_argument("--scores", action="store_true")
    ap.add_argument("--seconds", type=float, default=48.0)
    ap.add_argument("--sessions", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=150.0)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=str(HERE / "profiles" / "live_scores_timing.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = [("this_no_scores", HERE, False)]
    if a.parent_root:
        variants.append(("parent_no_scores", Path(a.parent_root).resolve(), False))
    variants.append(("this_scores", HERE, True))
    res = {"workload": f"wavlm_large_s80_md, 8 s windows at a 0.8 s step, seeded turn-taking weights, {a.seconds:g} s of the synthetic "
                       "recording (seed 3407) per session, 0.8 s per feed: every timed step completes one window per session",
           "clock": "host clock between two device synchronisations around feed() / tick(); the first session (hub) of a process "
                    "and the first window are untimed", "rounds": a.rounds, "order": [v[0] for v in variants]}
    for mode in ("solo", "hub"):
        rows = {v[0]: [] for v in variants}
        for _ in range(a.rounds):
            for name, root, scores in variants:                     # interleaved: the variants share the box's state
                row = run_child(root, mode, scores, a)
                rows[name].append(row)
                res["device"] = row["device"]
                print(mode, name, row, flush=True)
        res[mode] = {name: summary(v) for name, v in rows.items()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({m: {k: (v["mean_of_medians_ms"], v["spread_ms"]) for k, v in res[m].items()} for m in ("solo", "hub")}))


if __name__ == "__main__":
    main()
