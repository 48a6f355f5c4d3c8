"""tests/golden/scores_ref.npz: what the reference makes of powerset log-probabilities on its soft path (build container only:
needs the reference tree; the GPU box reads only the .npz).

    python scripts/gen_scores_golden.py           # write the golden
    python scripts/gen_scores_golden.py --check   # recompute and compare with the committed file (exit 1 on a difference)

Two families of cases (PA/ = pyannote-audio/pyannote/audio/):
  soft multilabel   the reference-made `logp` arrays the segmentation goldens store (tests/golden/seg_*.npz) through the
                    reference's own Powerset.to_multilabel(powerset, soft=True)                 PA/utils/powerset.py:103-128
  aggregation       seeded powerset logits -> log_softmax -> to_multilabel(soft=True) -> soft [C, L, S];
                    seeded hard clusters [C, S] (-2 = inactive);
                    clustered scores by SpeakerDiarization.reconstruct's own lines              PA/pipelines/speaker_diarization.py:400-423
                    (called with a shell whose to_diarization hands the clustered array back);
                    Inference.aggregate(clustered, frames, warm_up, hamming=True, missing=0.0)  PA/core/inference.py:544-666
                    crop(Segment(0, num_samples / sr), mode="loose") for a padded last window   PA/core/inference.py:400-403
`Powerset`, `reconstruct` and `Inference.aggregate` are the reference's own (oracle/ref_host.py imports them by path); the
crop is the pyannote.core stand-in's (oracle/pyannote_core_stub.py).
"""
from __future__ import annotations

import argparse
import math
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))

SR = 16000
L2S = 99                  # frames of a 2 s window
# the segmentation goldens whose reference-made log-probabilities get a soft-multilabel golden
ML_SOURCES = ("seg_tiny_ln", "seg_tiny_gn", "seg_wavlm_base_s80_md", "seg_wavlm_large_s80_md", "seg_wavlm_large",
              "seg_tt_tiny_ln", "seg_tt_tiny_gn", "seg_tt_wavlm_large_s80_md", "seg_outlier_tiny_ln", "seg_loud_tiny_gn")

# name: (seed, C, S, K, step ratio, padded last window, warm_up)
AGG_CASES = {
    "w2s_c12_s4_k5": (11, 12, 4, 5, 0.5, False, (0.0, 0.0)),
    "w2s_c23_s3_k2_deep": (12, 23, 3, 2, 0.1, False, (0.0, 0.0)),
    "w2s_c1": (13, 1, 4, 3, 0.5, False, (0.0, 0.0)),
    "w2s_k1": (14, 6, 3, 1, 0.5, False, (0.0, 0.0)),
    "w2s_k32": (15, 5, 8, 32, 0.5, False, (0.0, 0.0)),
    "w2s_c7_padded": (16, 7, 4, 4, 0.5, True, (0.0, 0.0)),
    "w2s_c12_warm_up": (17, 12, 4, 3, 0.1, True, (0.1, 0.1)),
}


def num_samples_for(C: int, window: int, step: int, padded: bool) -> int:
    """a recording length whose window plan (PA/core/inference.py:285-299) has C windows, the last zero-padded or not"""
    if not padded:
        return window + (C - 1) * step
    if C == 1:
        return window - step // 2
    return window + (C - 2) * step + step // 2


def seeded_hard(seed: int, C: int, S: int, K: int) -> np.ndarray:
    """hard clusters int8 [C, S]: every cluster 0 .. K-1 occurs, a quarter of the entries is -2 (inactive), windows 3 and 4
    (when there are that many, K > 1) have no local speaker in cluster 0 — with a step of half a window those are ALL the
    windows that cover the frames from the start of window 4 to the end of window 3"""
    g = np.random.default_rng(seed)
    hard = g.integers(0, K, size=(C, S)).astype(np.int8)
    hard[g.random((C, S)) < 0.25] = -2
    flat = hard.reshape(-1)
    slots = g.permutation(flat.size)[:K] if flat.size >= K else np.arange(flat.size)
    flat[slots] = np.arange(len(slots)) % K                   # every cluster has a slot
    if C > 4 and K > 1:
        rows = hard[3:5]
        rows[rows == 0] = 1
        if not (hard == 0).any():
            hard[0, 0] = 0
    return hard


def reference_soft(logits: np.ndarray, S: int, max_set: int = 2) -> np.ndarray:
    """seeded logits [C, L, n_classes] -> the reference's log_softmax + Powerset.to_multilabel(soft=True), float32"""
    import torch
    from oracle import ref_host
    ns = ref_host.load()
    powerset = ns.modules.inference.Powerset(S, max_set)
    logp = torch.nn.functional.log_softmax(torch.from_numpy(logits), dim=-1)      # the model's nn.LogSoftmax(dim=-1)
    return powerset.to_multilabel(logp, soft=True).numpy().astype(np.float32)


def agg_inputs(name: str):
    """-> (soft f32 [C, L, S], hard int8 [C, S], duration, step ratio, num_samples, warm_up)"""
    seed, C, S, K, ratio, padded, warm_up = AGG_CASES[name]
    from oracle import ref_host
    ns = ref_host.load()
    n_classes = ns.modules.inference.Powerset(S, 2).num_powerset_classes
    g = np.random.default_rng(seed)
    logits = (3.0 * g.standard_normal((C, L2S, n_classes))).astype(np.float32)
    window, step = int(math.floor(2.0 * SR)), int(round(ratio * 2.0 * SR))
    return reference_soft(logits, S), seeded_hard(seed, C, S, K), 2.0, ratio, num_samples_for(C, window, step, padded), warm_up


def reference_clustered(soft: np.ndarray, hard: np.ndarray, duration: float, ratio: float):
    """SpeakerDiarization.reconstruct's clustered segmentations (its own lines 400-423) as a SlidingWindowFeature"""
    from oracle import ref_host
    ns = ref_host.load()
    core = ns.core
    chunks = core.SlidingWindow(start=0.0, duration=duration, step=ratio * duration)
    shell = types.SimpleNamespace(to_diarization=lambda clustered, count: clustered)
    return ns.SpeakerDiarization.reconstruct(shell, core.SlidingWindowFeature(soft, chunks), hard, None)


def reference_scores(soft, hard, duration, ratio, num_samples, warm_up) -> np.ndarray:
    """the reference's clustered scores + aggregate (+ crop) on one case -> scores f32 [T, K]"""
    from oracle import ref_host
    ns = ref_host.load()
    core = ns.core
    window, step_n = int(math.floor(duration * SR)), int(round(ratio * duration * SR))
    has_last = (num_samples - window) % step_n > 0 if num_samples >= window else True
    clustered = reference_clustered(soft, hard, duration, ratio)
    assert clustered.data.dtype == np.float64
    frames = core.SlidingWindow(**ref_host.RECEPTIVE_FIELD)
    aggregated = ns.Inference.aggregate(clustered, frames, warm_up=tuple(warm_up), hamming=True, missing=0.0,
                                        skip_average=False)
    if has_last:
        aggregated.data = aggregated.crop(core.Segment(0.0, num_samples / SR), mode="loose")
    assert aggregated.data.dtype == np.float32
    return np.ascontiguousarray(aggregated.data)


def check_coverage(out) -> None:
    """what the aggregation cases must contain between them to pin anything"""
    hards = [out[f"{n}_hard"] for n in AGG_CASES]
    assert any((h == -2).any() for h in hards), "-2 entries"
    assert any(any(not (row == k).any() for row in h) for h in hards for k in range(int(h.max()) + 1)), "absent cluster"
    assert any(any(len(set(row[row >= 0].tolist())) < (row >= 0).sum() for row in h) for h in hards), "two locals, one cluster"
    # a cluster absent from every window covering some frame: its score there is `missing` = 0.0 while another column lives
    name = "w2s_c12_s4_k5"
    sc = out[f"{name}_scores"]
    dead = (sc[:, 0] == 0.0) & (sc[:, 1:].max(axis=1) > 0.0)
    assert dead[200:249].all(), "cluster 0 is absent from windows 3 and 4: frames 200 .. 248 have no entry"


def generate():
    out = {}
    for stem in ML_SOURCES:
        g = np.load(GOLD / f"{stem}.npz")
        logp = g["logp"]
        import torch
        from oracle import ref_host
        ns = ref_host.load()
        assert logp.shape[-1] == 11
        powerset = ns.modules.inference.Powerset(4, 2)
        out[f"{stem}_soft"] = powerset.to_multilabel(torch.from_numpy(logp), soft=True).numpy().astype(np.float32)
        out["mapping_4_2"] = powerset.mapping.numpy().astype(np.uint8)
        print(f"{stem}: soft {out[f'{stem}_soft'].shape}", flush=True)
    for name in AGG_CASES:
        soft, hard, dur, ratio, n, warm_up = agg_inputs(name)
        sc = reference_scores(soft, hard, dur, ratio, n, warm_up)
        out[f"{name}_soft"] = soft
        out[f"{name}_hard"] = hard
        out[f"{name}_args"] = np.array([dur, ratio, n, warm_up[0], warm_up[1]], dtype=np.float64)
        out[f"{name}_scores"] = sc
        assert sc.shape[1] == AGG_CASES[name][3] and np.isfinite(sc).all()
        print(f"{name}: soft {soft.shape}, K = {sc.shape[1]}, {len(sc)} frames, max {sc.max():.4f}, "
              f"{int((sc == 0.0).sum())} zeros", flush=True)
    check_coverage(out)
    out["ml_cases"] = np.array(ML_SOURCES)
    out["agg_cases"] = np.array(list(AGG_CASES))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed golden instead of writing it")
    a = ap.parse_args()
    out = generate()
    path = GOLD / "scores_ref.npz"
    if a.check:
        g = np.load(path)
        bad = [k for k in out if k not in g.files or not np.array_equal(np.asarray(out[k]), g[k])]
        bad += [k for k in g.files if k not in out]
        print("differences:", bad or "none")
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
