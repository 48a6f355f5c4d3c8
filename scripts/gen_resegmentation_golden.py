"""tests/golden/resegmentation_ref.npz: what the reference's Resegmentation pipeline makes of hard powerset decisions and a given
diarization (build container only: needs the reference tree; the GPU box reads only the .npz).

    python scripts/gen_resegmentation_golden.py           # write the golden
    python scripts/gen_resegmentation_golden.py --check   # recompute and compare with the committed file (exit 1 on a difference)

Per case, PA/pipelines/resegmentation.py:184-253 in its order, with the reference's own functions (PA/ = pyannote-audio/
pyannote/audio/; oracle/ref_host.py imports them by path, PA/utils/permutation.py is loaded here the same way):
    (binarize: the decisions are hard already)                       resegmentation.py:185-190
    SpeakerDiarizationMixin.speaker_count(warm_up=(w, w))            :193-197
    the hypothesis on the frame grid                                 :202-208   <- NOT the reference's: see below
    Inference.trim(warm_up=(w, w))                                   :212-214
    zero-pad to n = max(K, S) columns                                :217-228
    per window: diarization.crop(chunk)[:, :L'], permutate(mae)      :230-243
    SpeakerDiarizationMixin.to_diarization                           :246
    Binarize(0.5, 0.5, min_duration_on, 0.0)                         :249-253 (to_annotation without rename_tracks: RTTM has no tracks)
Two things are not the reference's.  (1) pyannote.core is not in this image, so Annotation.discretize is
postprocess.discretize_turns (a restatement; the matrix it gives is stored as an INPUT of the case, the boundary stays unpinned)
and SlidingWindowFeature.crop is the stand-in's (oracle/pyannote_core_stub.py).  (2) Where the last windows reach past the
support Segment(0, duration + step) the reference's crop comes back short and permutate refuses the shapes; the project counts
rows at or beyond Tr as inactive, so the matrix is extended with zero rows before the loop.

Uniqueness.  linear_sum_assignment's choice among equal-cost assignments is scipy's, and another build may choose differently.
For every window with n <= 6 all n! assignments are enumerated on the integer counts: every optimal one must pair the same
column CONTENTS as scipy's (exchanging reference columns that are identical inside the window, or identical local speakers, is
the only freedom); a case where a window fails this is refused and not written.

Cases: decisions of tests/golden/host_ref.npz (2, 5 and 8 s windows), the raw EN2002a decisions of detection_ref.npz and, once,
the 2241 windows of host30.npz; hypotheses derived from their own reference-made result (see VARIANTS), at warm_up 0 and 0.05.
"""
from __future__ import annotations

import argparse
import importlib.util
import itertools
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))

SR = 16000
VARIANTS = ("perm", "later", "earlier", "k2", "k6", "empty", "ghost")
WARM_UPS = (0.0, 0.05)


# ----------------------------------------------------------------------------- inputs
def decisions():
    """-> [(name, source "file.npz:key", seg, duration, ratio, num_samples, own result as RTTM text)]"""
    from scripts.gen_detection_golden import num_samples_for
    d = np.load(GOLD / "detection_ref.npz")
    h = np.load(GOLD / "host_ref.npz")
    out = []
    for name in ("w2s_c60", "w5s_c40_step50", "w8s_c7_cap1", "w8s_c1"):
        dur, ratio, n = d[f"{name}_args"]
        out.append((name, f"host_ref.npz:{name}_seg", h[f"{name}_seg"], float(dur), float(ratio), int(n),
                    h[f"{name}_rttm"].tobytes().decode()))
    dur, ratio, n = d["EN2002a_args"]
    out.append(("EN2002a", "detection_ref.npz:EN2002a_seg", d["EN2002a_seg"], float(dur), float(ratio), int(n),
                (GOLD / "e2e_EN2002a_30s.rttm").read_text()))
    h30 = np.load(GOLD / "host30.npz")
    out.append(("host30", "host30.npz:seg", h30["seg"], 8.0, 0.1, num_samples_for(len(h30["seg"]), 128000, 12800, False),
                h30["rttm"].tobytes().decode()))
    return out


def hypothesis(variant: str, turns, duration: float):
    """turns [(start, end, label)] of the decisions' own result -> the hypothesis of one variant"""
    labels = sorted({t[2] for t in turns}, key=str)
    if variant == "perm":                                   # the same turns under names whose sorted order is reversed
        names = {label: f"spk{len(labels) - 1 - k:02d}" for k, label in enumerate(labels)}
        return [(a, b, names[label]) for a, b, label in turns]
    if variant in ("later", "earlier"):                     # every boundary moved by 0.3 s
        d = 0.3 if variant == "later" else -0.3
        return [(max(a + d, 0.0), b + d, label) for a, b, label in turns if b + d > 0.0]
    if variant == "k2":                                     # the two speakers who talk most
        total = {label: sum(b - a for a, b, x in turns if x == label) for label in labels}
        keep = sorted(labels, key=lambda x: (-total[x], str(x)))[:2]
        return [t for t in turns if t[2] in keep]
    if variant == "k6":                                     # six speakers: the busiest label gives every other turn away
        out = list(turns)
        while len({t[2] for t in out}) < 6:
            cnt = {}
            for t in out:
                cnt[t[2]] = cnt.get(t[2], 0) + 1
            busiest = sorted(cnt, key=lambda x: (-cnt[x], str(x)))[0]
            new, k = f"split{len(cnt)}", 0
            if cnt[busiest] < 2:
                out.append((0.5 * duration, 0.5 * duration + 0.4, new))
                continue
            for i, t in enumerate(out):
                if t[2] == busiest:
                    if k % 2:
                        out[i] = (t[0], t[1], new)
                    k += 1
        return out
    if variant == "empty":
        return []
    if variant == "ghost":                                  # a speaker the decisions never show: one second in every five
        return list(turns) + [(s, s + 1.0, "zz_ghost") for s in np.arange(0.25, duration, 5.0).tolist()]
    raise ValueError(variant)


def to_rttm(turns, uri: str) -> str:
    """repr() keeps the float64 boundaries, so that the stored text parses back to the same turns"""
    return "".join(f"SPEAKER {uri} 1 {a!r} {b - a!r} <NA> <NA> {label} <NA> <NA>\n" for a, b, label in turns)


# ----------------------------------------------------------------------------- the reference's functions
def load_permutation(ns):
    """PA/utils/permutation.py by path, with the pyannote.core stand-in in sys.modules while it is imported"""
    from oracle import ref_host
    saved = {k: v for k, v in sys.modules.items() if k == "pyannote" or k.startswith("pyannote.")}
    try:
        for name in ("pyannote", "pyannote.core"):
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        sys.modules["pyannote.core"].SlidingWindowFeature = ns.core.SlidingWindowFeature
        spec = importlib.util.spec_from_file_location("pyannote_audio_utils_permutation", ref_host.PA / "utils" / "permutation.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k in [k for k in sys.modules if k == "pyannote" or k.startswith("pyannote.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mod


def check_unique(counts: np.ndarray, perms, ref_win: np.ndarray, seg_win: np.ndarray) -> bool:
    """one window, n <= 6: every assignment with the minimal integer total pairs the same column contents as `perms`
    (perms[i] = j: local speaker j goes to reference column i)"""
    n = counts.shape[0]
    rid = {}
    r = [rid.setdefault(ref_win[:, i].tobytes(), len(rid)) for i in range(n)]
    sid = {}
    s = [sid.setdefault(seg_win[:, j].tobytes(), len(sid)) for j in range(n)]
    allp = np.array(list(itertools.permutations(range(n))), dtype=np.int64)
    total = counts[np.arange(n)[None, :], allp].sum(axis=1)
    mine = int(sum(counts[i, perms[i]] for i in range(n)))
    if mine != int(total.min()):
        return False
    sig = sorted((r[i], s[perms[i]]) for i in range(n))
    return all(sorted((r[i], s[p[i]]) for i in range(n)) == sig for p in allp[total == total.min()])


def reference_resegmentation(ns, perm_mod, seg: np.ndarray, ref: np.ndarray, duration: float, ratio: float, w: float, uri: str):
    """resegmentation.py:184-253 -> dict of arrays, or None when a window's assignment is not unique"""
    from oracle import ref_host
    core = ns.core
    C, L, S = seg.shape
    chunks = core.SlidingWindow(start=0.0, duration=duration, step=ratio * duration)            # PA/core/inference.py:377-381
    frames = core.SlidingWindow(**ref_host.RECEPTIVE_FIELD)
    segmentations = core.SlidingWindowFeature(seg.astype(np.float32), chunks)
    count = ns.Mixin.speaker_count(segmentations, frames, warm_up=(w, w))                          # :193-197
    trimmed = ns.Inference.trim(segmentations, warm_up=(w, w))                                      # :212-214
    Lt = trimmed.data.shape[1]
    last = trimmed.sliding_window[C - 1]
    need = frames.crop(last, mode="loose", return_ranges=True)[0][0] + Lt + 1
    data = np.zeros((max(len(ref), need), ref.shape[1]), dtype=np.uint8)                            # (2) of the module docstring
    data[:len(ref)] = ref
    diarization = core.SlidingWindowFeature(data, frames)
    num_speakers = diarization.data.shape[1]                                                        # :217-228
    if num_speakers > S:
        trimmed.data = np.pad(trimmed.data, ((0, 0), (0, 0), (0, num_speakers - S)))
    elif num_speakers < S:
        diarization.data = np.pad(diarization.data, ((0, 0), (0, S - num_speakers)))
        num_speakers = S
    n = num_speakers
    permutated = np.full_like(trimmed.data, np.nan)                                                 # :231-243
    counts = np.zeros((C, n, n), dtype=np.int32)
    hard = np.zeros((C, S), dtype=np.int8)
    for c, (chunk, segmentation) in enumerate(trimmed):
        local = diarization.crop(chunk)[np.newaxis, :Lt]
        (permutated[c],), (perm,), (cost,) = perm_mod.permutate(local, segmentation, cost_func=perm_mod.mae_cost_func,
                                                                return_cost=True)
        assert cost.dtype == np.float32 and None not in perm
        cnt = np.rint(cost.astype(np.float64) * Lt).astype(np.int32)
        # the definition of the issue: cost = float32(count) / float32(L'), count the exact number of differing frames
        assert np.array_equal(cnt, np.count_nonzero(local[0][:, :, None] != segmentation[:, None, :], axis=0)), (uri, c)
        assert np.array_equal(cnt.astype(np.float32) / np.float32(Lt), cost), (uri, c)
        counts[c] = cnt
        if n <= 6 and not check_unique(cnt, perm, local[0], segmentation):
            print(f"  {uri}: window {c} has more than one optimal assignment - refused", flush=True)
            return None
        for i, j in enumerate(perm):
            if j < S:
                hard[c, j] = i
    discrete, _ = ns.Mixin.to_diarization(core.SlidingWindowFeature(permutated, trimmed.sliding_window), count)   # :246
    ann = ns.Binarize(onset=0.5, offset=0.5, min_duration_on=0.0, min_duration_off=0.0)(discrete)   # :249-253
    ann.uri = uri
    sw = discrete.sliding_window
    return dict(counts=counts, hard=hard, permutated=permutated[:, :, :].astype(np.uint8), count=count.data.astype(np.uint8),
                discrete=discrete.data.astype(np.uint8), frames=np.array([sw.start, sw.duration, sw.step]),
                rttm=np.frombuffer(ann.to_rttm().encode(), dtype=np.uint8))


def generate():
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.der import parse_rttm
    from diarizen_amd.postprocess import discretize_turns, receptive_field, reference_extent
    from oracle import ref_host
    ns = ref_host.load()
    perm_mod = load_permutation(ns)
    out, names, refused = {}, [], []
    for name, src, seg, dur, ratio, num_samples, own in decisions():
        turns = parse_rttm(own)
        chunks = SlidingWindow(start=0.0, duration=dur, step=ratio * dur)
        _, Tr = reference_extent(num_samples, SR, chunks, receptive_field(SR))
        for variant in (VARIANTS if name != "host30" else ("perm",)):
            hyp = to_rttm(hypothesis(variant, turns, num_samples / SR), name)
            ref, labels = discretize_turns(parse_rttm(hyp), receptive_field(SR), Tr)
            for w in (WARM_UPS if name != "host30" else (0.0,)):
                case = f"{name}_{variant}_w{int(round(w * 100)):02d}"
                res = reference_resegmentation(ns, perm_mod, seg, ref, dur, ratio, w, case)
                if res is None:
                    refused.append(case)
                    continue
                names.append(case)
                out[f"{case}_src"] = np.array(src)
                out[f"{case}_args"] = np.array([dur, ratio, num_samples, w], dtype=np.float64)
                out[f"{case}_hypothesis"] = np.frombuffer(hyp.encode(), dtype=np.uint8)
                out[f"{case}_labels"] = np.array([str(x) for x in labels], dtype=str)
                out[f"{case}_ref"] = ref
                for k, v in res.items():
                    out[f"{case}_{k}"] = v
                print(f"{case}: C={len(seg)} K={len(labels)} Tr={Tr} frames={len(res['discrete'])} "
                      f"regions={len(res['rttm'].tobytes().splitlines())}", flush=True)
    out["cases"] = np.array(names)
    out["refused"] = np.array(refused, dtype=str)
    print(f"{len(names)} cases, refused: {refused or 'none'}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed golden instead of writing it")
    a = ap.parse_args()
    out = generate()
    path = GOLD / "resegmentation_ref.npz"
    if a.check:
        g = np.load(path)
        bad = [k for k in out if k not in g.files or not np.array_equal(np.asarray(out[k]), g[k])]
        print("differences:", bad or "none")
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
