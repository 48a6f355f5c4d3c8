"""tests/golden/detection_ref.npz: what the reference's voice activity / overlapped speech detection pipelines make of hard
powerset decisions (build container only: needs the reference tree; the GPU box reads only the .npz).

    python scripts/gen_detection_golden.py           # write the golden
    python scripts/gen_detection_golden.py --check   # recompute and compare with the committed file (exit 1 on a difference)

Per file the two pipelines run (PA/ = pyannote-audio/pyannote/audio/):
    hard multilabel decisions [C, L, S]                       Powerset.to_multilabel(soft=False), PA/utils/powerset.py:103-130
    pre-aggregation hook                                      VAD: max over speakers, PA/pipelines/voice_activity_detection.py:125
                                                              OSD: 2nd largest,       PA/pipelines/overlapped_speech_detection.py:132
    Inference.aggregate(hamming=True, missing=0.0, warm_up)   PA/core/inference.py:389-397, 544-666 (warm_up (0, 0): DiariZen)
    crop(Segment(0, num_samples / sr), mode="loose")          PA/core/inference.py:400-403 (padded last window only)
    Binarize(onset=0.5, offset=0.5, 0.0, 0.0)                 PA/utils/signal.py:207-317, onset / offset of powerset models
    uri + relabel to SPEECH / OVERLAP                         voice_activity_detection.py:219, overlapped_speech_detection.py:235
`Inference.aggregate` and `Binarize` are the reference's own (oracle/ref_host.py imports them by path); the hooks are the
two one-line reductions quoted above, the crop is the pyannote.core stand-in's (oracle/pyannote_core_stub.py).

Cases: the decision arrays of tests/golden/host_ref.npz (2, 5 and 8 s windows, S = 3 and 4, with the zero-padded last window
of a recording whose length is not on the step grid), those of tests/golden/host30.npz (2241 windows), planted arrays whose
frames hit exactly 0.5 (two windows at mirrored Hamming positions, one active) and must keep their state, and the raw
(median filter off) decisions of tests/golden/EN2002a_30s.wav with the seeded turn-taking weights: the oracle's
reference-ordered segmentation forward (oracle/seg_model.py) + the reference's Powerset.
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))

SR = 16000
TASKS = ("speech", "overlap")
LABELS = {"speech": "SPEECH", "overlap": "OVERLAP"}


def hook(task, scores):
    """the pre-aggregation hooks of the two pipelines on [C, L, S] scores"""
    if task == "speech":
        return np.max(scores, axis=-1, keepdims=True)                   # voice_activity_detection.py:125
    return np.partition(scores, -2, axis=-1)[:, :, -2, np.newaxis]      # overlapped_speech_detection.py:132


def num_samples_for(C: int, window: int, step: int, padded: bool) -> int:
    """a recording length whose window plan (PA/core/inference.py:285-299) has C windows, the last zero-padded or not"""
    if not padded:
        return window + (C - 1) * step
    if C == 1:
        return window - step // 2
    return window + (C - 2) * step + step // 2


def planted(seed: int, C: int, L: int, S: int, shift: int):
    """seeded decisions (oracle/gen_golden.py:synth_decisions) with, for every pair of neighbouring windows, the frame they
    both cover at mirrored positions a, L-1-a (the Hamming window is symmetric: equal weights) set to "one window active, the
    other not": its score is exactly 0.5 in float32 and Binarize keeps the previous state.  The frame before it is set to the
    same decision in both windows, active or not, so both kept states occur; k = 2 active speakers make it an overlap tie too."""
    from oracle.gen_golden import synth_decisions
    g = np.random.default_rng(seed)
    seg, _ = synth_decisions(seed, C, L, S, 2)
    a = (L - 1 + shift) // 2                 # frame start_c + a of window c is frame b = a - shift of window c + 1
    b = a - shift
    assert a + b == L - 1
    for c in range(C - 1):
        prev = g.random() < 0.5
        k = int(g.integers(1, 3))
        for w, l in ((c, a - 1), (c + 1, b - 1)):
            seg[w, l, :] = 0
            if prev:
                seg[w, l, :k] = 1
        on, off = ((c, a), (c + 1, b)) if g.random() < 0.5 else ((c + 1, b), (c, a))
        seg[on[0], on[1], :] = 0
        seg[on[0], on[1], :k] = 1
        seg[off[0], off[1], :] = 0
    return seg


def load_cases(e2e: bool = True):
    """-> list of (name, seg [C, L, S] u8, duration s, step ratio, num_samples, source) ; source = where seg is stored"""
    h = np.load(GOLD / "host_ref.npz")
    cases = []
    for i, name in enumerate(str(c) for c in h["cases"]):
        seg = h[f"{name}_seg"]
        dur, ratio, _ = h[f"{name}_args"]
        window, step = int(math.floor(dur * SR)), int(round(ratio * dur * SR))
        cases.append((name, seg, float(dur), float(ratio), num_samples_for(seg.shape[0], window, step, i % 2 == 0),
                      f"host_ref.npz:{name}_seg"))
    h30 = np.load(GOLD / "host30.npz")
    seg = h30["seg"]
    cases.append(("host30", seg, 8.0, 0.1, num_samples_for(seg.shape[0], 128000, 12800, False), "host30.npz:seg"))
    # planted ties: 2 s windows (L = 99), step 1 s = 50 frames: every frame is covered by at most two windows
    for name, seed, C, S in (("tie_w2s_c12", 5, 12, 4), ("tie_w2s_c9_s3", 6, 9, 3)):
        cases.append((name, planted(seed, C, 99, S, 50), 2.0, 0.5, num_samples_for(C, 32000, 16000, seed % 2 == 0), "here"))
    if e2e:
        seg, n = e2e_decisions()
        cases.append(("EN2002a", seg, 8.0, 0.1, n, "here"))
    return cases


def e2e_decisions():
    """raw hard decisions of tests/golden/EN2002a_30s.wav, 8 s windows, step 0.8 s, zero-padded last window: the oracle's
    segmentation forward (reference order, oracle/seg_model.py) + the reference's own Powerset.to_multilabel(soft=False)"""
    import torch
    from oracle import ref_host, seg_model
    from oracle.configs import get_seg_config
    from oracle.pipeline import slide_windows
    from oracle.wav import first_channel_pcm16
    from testkit.weights import turn_taking_state_dict
    ns = ref_host.load()
    cfg = get_seg_config("wavlm_large_s80_md")
    sd = turn_taking_state_dict(cfg, 0)
    wave = torch.from_numpy(first_channel_pcm16(str(GOLD / "EN2002a_30s.wav")))
    chunks = slide_windows(wave, 128000, 12800)
    powerset = ns.modules.inference.Powerset(cfg.max_speakers_per_chunk, cfg.max_speakers_per_frame)
    out = []
    for c0 in range(0, chunks.shape[0], 4):
        logp = seg_model.seg_forward(sd, cfg, chunks[c0:c0 + 4])
        out.append(powerset.to_multilabel(logp, soft=False).numpy())
        print(f"  e2e windows {min(c0 + 4, chunks.shape[0])}/{chunks.shape[0]}", flush=True)
    return np.vstack(out).astype(np.uint8), int(wave.numel())


def reference_detection(seg: np.ndarray, duration: float, ratio: float, num_samples: int, task: str, uri: str):
    """the reference's aggregate + crop + Binarize on one case -> (scores [T, 1] f32, activity [T] u8, RTTM text)"""
    from oracle import ref_host
    ns = ref_host.load()
    core = ns.core
    C = seg.shape[0]
    step = ratio * duration
    window, step_n = int(math.floor(duration * SR)), int(round(ratio * duration * SR))
    has_last = (num_samples - window) % step_n > 0 if num_samples >= window else True
    assert (num_samples - window) // step_n + 1 + int(has_last) == C if num_samples >= window else C == 1
    outputs = hook(task, seg.astype(np.float32))
    frames = core.SlidingWindow(**ref_host.RECEPTIVE_FIELD)
    aggregated = ns.Inference.aggregate(core.SlidingWindowFeature(outputs, core.SlidingWindow(start=0.0, duration=duration,
                                                                                              step=step)),
                                        frames, warm_up=(0.0, 0.0), hamming=True, missing=0.0)
    if has_last:
        aggregated.data = aggregated.crop(core.Segment(0.0, num_samples / SR), mode="loose")
    ann = ns.Binarize(onset=0.5, offset=0.5, min_duration_on=0.0, min_duration_off=0.0)(aggregated)
    ann.uri = uri
    for tracks in ann._tracks.values():                 # rename_labels({label: "SPEECH" / "OVERLAP"})
        for tr in tracks:
            tracks[tr] = LABELS[task]
    # the activity the state machine went through, frame by frame (regions cover frame middles t_start .. t_end)
    y = aggregated.data[:, 0]
    act = np.zeros(len(y), dtype=np.uint8)
    state = y[0] > 0.5
    act[0] = state
    for i in range(1, len(y)):
        if state and y[i] < 0.5:
            state = False
        elif not state and y[i] > 0.5:
            state = True
        act[i] = state
    return aggregated.data.astype(np.float32), act, ann.to_rttm()


def generate():
    out, names = {}, []
    for name, seg, dur, ratio, n, src in load_cases():
        names.append(name)
        out[f"{name}_args"] = np.array([dur, ratio, n], dtype=np.float64)
        out[f"{name}_src"] = np.array(src)
        if src == "here":
            out[f"{name}_seg"] = seg
        for task in TASKS:
            sc, act, rttm = reference_detection(seg, dur, ratio, n, task, name)
            ties = int((sc[:, 0] == np.float32(0.5)).sum())
            out[f"{name}_{task}_scores"] = sc
            out[f"{name}_{task}_active"] = act
            out[f"{name}_{task}_rttm"] = np.frombuffer(rttm.encode(), dtype=np.uint8)
            out[f"{name}_{task}_ties"] = np.int64(ties)
            print(f"{name} {task}: {len(sc)} frames, {ties} exact 0.5 ties, {int(act.sum())} active, "
                  f"{len(rttm.splitlines())} regions", flush=True)
    for name in names:
        if name.startswith("tie_"):
            for task in TASKS:
                sc, act = out[f"{name}_{task}_scores"][:, 0], out[f"{name}_{task}_active"]
                tie = np.nonzero(sc == np.float32(0.5))[0]
                assert len(tie) and np.array_equal(act[tie], act[tie - 1]), (name, task)
                assert act[tie].min() == 0 and act[tie].max() == 1, (name, task, "both kept states must occur")
    out["cases"] = np.array(names)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed golden instead of writing it")
    a = ap.parse_args()
    out = generate()
    path = GOLD / "detection_ref.npz"
    if a.check:
        g = np.load(path)
        bad = [k for k in out if not np.array_equal(np.asarray(out[k]), g[k])]
        print("differences:", bad or "none")
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
