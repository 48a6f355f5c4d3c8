"""Engine reuse: what a call returns depends on that call's inputs alone.  Shared by test_engine_reuse_gpu.py (the device
handle) and test_engine_reuse_host.py (a CPU model of a handle and six subtly wrong variants of it).  numpy / torch-CPU
only; nothing here touches a device.

A production handle is created once at the largest size and then called for hours with ragged last batches, other window
lengths and whatever audio arrives.  What it keeps from one forward to the next (csrc/engine.cpp): tables keyed by a
geometry (`ensure_pos_rowoff` by (L, rowD), `ensure_table` by L, `emb_set_geometry` by T with at most 64 geometries and
the image borders re-zeroed only on a change of T), |max| tracker arrays strided by max_batch and reset per call, and
workspaces that are zeroed at creation and never again.  A SCRIPT is a list of calls played on one oversize handle
(max_batch 6, max_samples 16000); `check_script` holds its outputs to

  (a) history   a shape run again after other shapes, loud audio, silence and other audio gives the bits it gave first;
  (b) size      the oversize handle gives the bits of a handle created at exactly (B, N);
  (c) parity    every call against the float64 oracle at the project's end-to-end bars;
  (d) subset    windows without an active speaker give seg_1's bias and the skip counters advance by exactly those windows;
  (e) geometry  the 65th distinct window length is refused, nothing is launched, the handle stays usable;
  (f) isolation a non-finite window changes no bit of its neighbours, in its own call or in the next one.

The shape tables are derived from the configuration (frame counts through the conv kernels and strides), not typed in:
`seg_table` / `emb_table` pick the smallest N and B for each target and the host test asserts every target is hit.
"""
from __future__ import annotations

import re
from contextlib import contextmanager

import numpy as np
import torch
import torch.nn.functional as F

PRECISIONS = ("f32", "f32s", "f32h", "f16")
SEG_CONFIGS = ("tiny_ln", "tiny_gn")
EMB_CONFIG = "tiny_ln"              # the ResNet trunk does not depend on the segmentation configuration
MAX_BATCH, MAX_SAMPLES = 6, 16000
S_MASKS = 3
MAX_GEOMS = 64                      # geometries one handle keeps (engine.cpp: emb_set_geometry)

SEG_L_TARGETS = (1, 2, 4, 49)
SEG_ROW_TARGETS = (1, 2, 127, 128, 129, 294)      # B * L around the 128-row tile; 127 is prime and > 49: the nearest reachable below
EMB_T_TARGETS = (8, 9, 17, 98)                    # stage widths 8/4/2/1, 9/5/3/2, 17/9/5/3, 98/49/25/13
EMB_B_TARGETS = (1, 2, 6)
GEOM_T0 = 8

MARGIN = 2e-3                       # argmax may differ where the float64 top-2 margin is below twice the log-prob bar ...
MAX_EXCLUDED = 0.01                 # ... on at most this share of a script's frames
BARS = {"f32": (1e-3, 1.0, 0.9999), "f32s": (1e-3, 1.0, 0.9999), "f32h": (1e-3, 1.0, 0.9999),
        "f16": (5e-2, 0.995, 0.999)}            # (max |d logp|, argmax agreement, embedding cosine): SURVEY 8d, tests/test_emb_gpu.py
F16_WAIVE_FRAMES = 50               # test_seg_loudness_extremes_in_one_batch: no agreement share below 50 frames


# ------------------------------------------------------------------ geometry
def seg_frames(cfg, N: int) -> int:
    n = N
    for k, s in zip(cfg.conv_kernels, cfg.conv_strides):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def emb_frames(N: int) -> int:
    return 1 + (N - 400) // 160 if N >= 400 else 0


def _smallest_n(frames, limit=MAX_SAMPLES):
    """{frame count: smallest N <= limit that gives it}"""
    out = {}
    for N in range(400, limit + 1):
        out.setdefault(frames(N), N)
    return out


_TABLES = {}


def seg_table(cfg):
    """[(B, N)]: every per-call frame count of SEG_L_TARGETS, every row count B * L of SEG_ROW_TARGETS (the nearest
    reachable one below where B <= MAX_BATCH, L <= L(MAX_SAMPLES) cannot factor it), ending with the handle's own size."""
    if ("seg", cfg.name) in _TABLES:
        return _TABLES[("seg", cfg.name)]
    n_for = _smallest_n(lambda N: seg_frames(cfg, N))
    Lmax = seg_frames(cfg, MAX_SAMPLES)
    shapes = [(1, n_for[L]) for L in SEG_L_TARGETS if L < Lmax]
    for rows in SEG_ROW_TARGETS:
        r = rows
        while True:
            fit = [(B, r // B) for B in range(1, MAX_BATCH + 1) if r % B == 0 and r // B <= Lmax]
            if fit:
                break
            r -= 1
        B, L = fit[0]
        shapes.append((B, MAX_SAMPLES if (B, L) == (MAX_BATCH, Lmax) else n_for[L]))
    out = []
    for s in shapes:
        if s not in out:
            out.append(s)
    full = (MAX_BATCH, MAX_SAMPLES)
    out = [s for s in out if s != full] + [full]
    _TABLES[("seg", cfg.name)] = out
    return out


def emb_table():
    """[(B, N)]: the T of EMB_T_TARGETS at the smallest N, batch sizes of EMB_B_TARGETS in turn, the widest at the largest batch"""
    shapes = []
    for i, T in enumerate(EMB_T_TARGETS):
        B = MAX_BATCH if T == max(EMB_T_TARGETS) else EMB_B_TARGETS[i % len(EMB_B_TARGETS)]
        shapes.append((B, 400 + 160 * (T - 1)))
    return shapes


# ------------------------------------------------------------------ fixed choices: weights, audio, masks
_WEIGHTS = {}


def get_cfg(name):
    from diarizen_amd.configs import get_seg_config
    return get_seg_config(name)


def seg_weights(name):
    if name not in _WEIGHTS:
        from testkit.weights import turn_taking_state_dict
        _WEIGHTS[name] = turn_taking_state_dict(get_cfg(name), 0)
    return _WEIGHTS[name]


def emb_weights():
    if "emb" not in _WEIGHTS:
        from testkit.weights import emb_state_dict
        _WEIGHTS["emb"] = emb_state_dict(0)
    return _WEIGHTS["emb"]


def _double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def audio(B, N, seed):
    from oracle.gen_golden import synth_wave
    return synth_wave(B, N, seed).contiguous()


def make_masks(cfg, B, N, seed):
    """[B, S_MASKS, L] of 0 / 1, L the segmentation frame count of N"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, S_MASKS, seg_frames(cfg, N), generator=g) > 0.3).float()


# ------------------------------------------------------------------ float64 references, computed once per input
_REFS = {}


@contextmanager
def _float64_default():
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


def reference(script, call):
    """float64 oracle output of a call: logp [B, L, C] or embeddings [B, S, 256]; None for a call that must be refused"""
    if call.get("expect") == "raise":
        return None
    src = script["calls"][call["ref_of"]] if "ref_of" in call else call
    key = (script["config"], src["rid"])
    if key not in _REFS:
        from oracle import emb_model, seg_model
        wave = _views(src).double()
        # the seeded weights are drawn in float32 and then widened: drawn under a float64 default they are other weights
        sd = _double(seg_weights(script["config"]) if src["kind"] == "seg" else emb_weights())
        with _float64_default():
            if src["kind"] == "seg":
                r = seg_model.seg_forward(sd, get_cfg(script["config"]), wave)
            else:
                r = emb_model.emb_forward(sd, wave, src["masks"].double())
        _REFS[key] = r.numpy()
    return _REFS[key]


def _views(call):
    """the [B, N] windows of a call, dense"""
    if call["kind"] == "emb_strided":
        return call["rec"].as_strided((call["B"], call["N"]), (call["stride"], 1)).contiguous()
    return call["wave"]


# ------------------------------------------------------------------ scripts
def _seg_call(B, N, seed, phase, **kw):
    return dict(kind="seg", B=B, N=N, wave=audio(B, N, seed), rid=("seg", B, N, seed), key=("seg", B, N), phase=phase, **kw)


def _emb_call(cfg, B, N, seed, phase, **kw):
    return dict(kind="emb", B=B, N=N, wave=audio(B, N, seed), masks=make_masks(cfg, B, N, seed + 500),
                rid=("emb", B, N, seed), key=("emb", B, N), phase=phase, **kw)


def _dirty(call, make):
    """three full-size calls between the passes: the last shape's audio at gain 1e4 (tiny_gn has no waveform
    normalisation), digital silence, other audio"""
    loud, quiet, other = dict(call), dict(call), make(MAX_BATCH, MAX_SAMPLES, 999, "dirty")
    loud.update(wave=call["wave"] * 1e4, rid=call["rid"] + ("x1e4",), key=call["key"] + ("x1e4",), phase="dirty", fit=False)
    quiet.update(wave=torch.zeros_like(call["wave"]), rid=call["rid"] + ("zeros",), key=call["key"] + ("zeros",), phase="dirty", fit=False)
    other.update(key=other["key"] + ("other",), fit=False)
    return [loud, quiet, other]


def _script(name, config, calls):
    return dict(name=name, config=config, max_batch=MAX_BATCH, max_samples=MAX_SAMPLES, calls=calls)


def seg_history(config):
    cfg = get_cfg(config)
    table = seg_table(cfg)
    first = [_seg_call(B, N, 100 + i, "first", fit=True) for i, (B, N) in enumerate(table)]
    second = [dict(c, phase="second") for c in reversed(first)]
    return _script("seg_history", config, first + _dirty(first[-1], _seg_call) + second)


def emb_history():
    cfg = get_cfg(EMB_CONFIG)

    def make(B, N, seed, phase, **kw):
        return _emb_call(cfg, B, N, seed, phase, **kw)
    first = [make(B, N, 200 + i, "first", fit=True) for i, (B, N) in enumerate(emb_table())]
    full = make(MAX_BATCH, MAX_SAMPLES, 210, "first", fit=True)
    first.append(full)
    second = [dict(c, phase="second") for c in reversed(first)]
    calls = first + _dirty(full, make) + second
    # leg a: the shared frame grid (melg) alternates with the dense path (fb) at one T
    B, N, q = MAX_BATCH, 400 + 160 * (EMB_T_TARGETS[2] - 1), 4
    rec = audio(1, (B - 1) * q * 160 + N, 220)[0].contiguous()
    masks = make_masks(cfg, B, N, 720)
    strided = dict(kind="emb_strided", B=B, N=N, stride=q * 160, rec=rec, masks=masks, rid=("emb_strided", B, N, q),
                   key=("emb_strided", B, N), phase="first")
    dense = dict(kind="emb", B=B, N=N, wave=_views(strided), masks=masks, rid=("emb_dense", B, N, q), key=("emb_dense", B, N),
                 phase="first", same_as=len(calls), fit=True)
    calls += [strided, dense, dict(strided, phase="second")]
    # legs b, c: windows 1 and 4 silent right after a call in which they were active, then active again
    active = make(MAX_BATCH, MAX_SAMPLES, 230, "first", fit=True)
    active.update(key=("leg_c",))
    silent = dict(active, masks=active["masks"].clone(), rid=active["rid"] + ("silent",), key=("leg_b",), fit=False,
                  skipped=(1, 4))
    silent["masks"][[1, 4]] = 0.0
    calls += [active, silent, dict(active, phase="second")]
    return _script("emb_history", EMB_CONFIG, calls)


def emb_geometries():
    cfg = get_cfg(EMB_CONFIG)
    Ts = list(range(GEOM_T0, GEOM_T0 + MAX_GEOMS))
    calls = [_emb_call(cfg, 1, 400 + 160 * (T - 1), 300 + T, "first") for T in Ts]
    refused = _emb_call(cfg, 1, 400 + 160 * (Ts[-1] + 1 - 1), 399, "refused", expect="raise")
    calls.append(refused)
    calls += [dict(calls[0], phase="second"), dict(calls[len(Ts) - 1], phase="second")]
    return _script("emb_geometries", EMB_CONFIG, calls)


POISON_WINDOW = 2


def _poisons(wave):
    out = {}
    for name in ("nan", "inf", "3e38"):
        w = wave.clone()
        if name == "nan":
            w[POISON_WINDOW, wave.shape[1] // 3] = float("nan")
        elif name == "inf":
            w[POISON_WINDOW, wave.shape[1] // 2] = float("inf")
        else:
            w[POISON_WINDOW] = 3e38
        out[name] = w
    return out


def poison(kind, config):
    cfg = get_cfg(config)
    B, N = 4, MAX_SAMPLES
    clean = _seg_call(B, N, 400, "first") if kind == "seg" else _emb_call(cfg, B, N, 400, "first")
    clean.update(key=("clean",))
    calls = [clean]
    for name, w in _poisons(clean["wave"]).items():
        calls.append(dict(clean, wave=w, rid=clean["rid"] + (name,), key=("poison", name), phase="poison", ref_of=0,
                          poisoned=POISON_WINDOW))
        calls.append(dict(clean, phase="second"))
    return _script(f"poison_{kind}", config, calls)


# ------------------------------------------------------------------ the driver
def _play(eng, call):
    """one call -> {"raised": exception or None, arrays by name, "stats": skip-counter advance of an embedding call}"""
    out = {"raised": None}
    try:
        if call["kind"] == "seg":
            out.update(eng.segment(call["wave"]))
            return out
        before = eng.skip_stats()
        if call.get("expect") == "raise":
            sentinel = torch.full((call["B"], S_MASKS, 256), -12345.0)
            out["sentinel"] = sentinel
            try:
                eng.embed(call["wave"], call["masks"], out=sentinel)
            finally:
                out["sentinel_after"] = sentinel.numpy().copy()
        elif call["kind"] == "emb_strided":
            out["emb"] = eng.embed_strided(call["rec"], call["B"], call["N"], call["stride"], call["masks"])
        else:
            out["emb"] = eng.embed(call["wave"], call["masks"])
        after = eng.skip_stats()
        out["stats"] = (after[0] - before[0], after[1] - before[1])
    except Exception as e:  # noqa: BLE001  (the check decides whether it was expected)
        out["raised"] = e
    return out


def run_script(make_engine, script, fit_cache=None):
    """Plays `script` on ONE handle from make_engine(max_batch, max_samples) and every call marked `fit` on a handle of
    exactly its size (cached in fit_cache by the call's input id).  The engine object has segment(wave) -> {"logp", "ml",
    "soft"}, embed(wave, masks, out=None) -> array, embed_strided(rec, B, N, stride, masks) -> array, skip_stats(), close();
    inputs are CPU tensors, outputs numpy arrays."""
    fit_cache = {} if fit_cache is None else fit_cache
    eng = make_engine(script["max_batch"], script["max_samples"])
    try:
        outs = [_play(eng, c) for c in script["calls"]]
    finally:
        eng.close()
    fits = {}
    for c in script["calls"]:
        if c.get("fit") and c["rid"] not in fits:
            if c["rid"] not in fit_cache:
                one = make_engine(c["B"], c["N"])
                try:
                    fit_cache[c["rid"]] = _play(one, c)
                finally:
                    one.close()
            fits[c["rid"]] = fit_cache[c["rid"]]
    return {"outs": outs, "fits": fits}


# ------------------------------------------------------------------ the checks
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(x, y, names):
    """names of the arrays that differ in any bit"""
    return [n for n in names if x.get(n) is None or y.get(n) is None or x[n].shape != y[n].shape
            or not np.array_equal(_bits(x[n]), _bits(y[n]))]


def _names(call):
    return ("logp", "ml", "soft") if call["kind"] == "seg" else ("emb",)


def _window_rows(a, skip):
    return np.delete(a, skip, axis=0) if skip is not None else a


def margin_stats(script):
    """(frames whose float64 top-2 margin is below MARGIN, frames, classes the float64 decisions take) over a segmentation script"""
    low = total = 0
    classes = set()
    for c in script["calls"]:
        ref = reference(script, c)
        if c["kind"] != "seg" or ref is None:
            continue
        ref = _window_rows(ref, c.get("poisoned"))
        top = np.sort(ref, axis=-1)
        low += int(((top[..., -1] - top[..., -2]) < MARGIN).sum())
        total += ref.shape[0] * ref.shape[1]
        classes |= set(np.unique(ref.argmax(-1)).tolist())
    return low, total, classes


def check_script(script, result, precision, bias=None, error_type=Exception):
    """Every assertion on a played script, (a) ... (f) of the module docstring; raises ONE AssertionError that lists every
    contract missed, each line starting with its letter.  Returns the worst parity figures."""
    from oracle import seg_model
    calls, outs, fits = script["calls"], result["outs"], result["fits"]
    bar_logp, bar_agree, bar_cos = BARS[precision]
    cfg = get_cfg(script["config"])
    fails = []
    worst = {"dlogp": 0.0, "agree": 1.0, "cos": 1.0, "excluded": 0, "frames": 0}
    first = {}
    for i, (c, o) in enumerate(zip(calls, outs)):
        tag = f"call {i} {c['kind']} B={c['B']} N={c['N']} [{c['phase']}]"
        # (e) the refusal
        if c.get("expect") == "raise":
            e = o["raised"]
            if e is None or not isinstance(e, error_type) or not re.search("too many distinct window lengths", str(e)):
                fails.append(f"(e) geometry: {tag} was not refused as the {MAX_GEOMS + 1}th window length: {e!r}")
            if not np.array_equal(_bits(o["sentinel_after"]), _bits(np.full_like(o["sentinel_after"], -12345.0))):
                fails.append(f"(e) geometry: {tag} wrote to its output buffer although it was refused")
            continue
        if o["raised"] is not None:
            fails.append(f"(e) usable: {tag} raised {o['raised']!r}")
            continue
        names = _names(c)
        skip = c.get("poisoned")
        # (a) history: the same input gave these bits the first time
        if c["key"] in first and c["phase"] == "second":
            bad = _same(outs[first[c["key"]]], o, names)
            if bad:
                fails.append(f"(a) history: {tag} differs from call {first[c['key']]} on the same input in {bad}")
        first.setdefault(c["key"], i)
        if "same_as" in c:
            bad = _same(outs[c["same_as"]], o, names)
            if bad:
                fails.append(f"(a) history: {tag} differs from call {c['same_as']} (same windows, other fbank path) in {bad}")
        # (b) size: the handle of exactly this size
        if c.get("fit"):
            f = fits[c["rid"]]
            if f["raised"] is not None:
                fails.append(f"(b) size: the exact-fit handle of {tag} raised {f['raised']!r}")
            else:
                bad = _same(f, o, names)
                if bad:
                    fails.append(f"(b) size: {tag} on the oversize handle differs from the exact-fit handle in {bad}")
        # (f) isolation: the healthy windows of a poisoned call have the clean call's bits
        if skip is not None:
            clean = outs[c["ref_of"]]
            bad = [n for n in names if not np.array_equal(_bits(_window_rows(o[n], skip)), _bits(_window_rows(clean[n], skip)))]
            if bad:
                fails.append(f"(f) isolation: {tag}: windows next to the non-finite one changed in {bad}")
        # (d) subset
        if c["kind"] != "seg":
            silent = [b for b in range(c["B"]) if not bool(c["masks"][b].any())]
            if "skipped" in c and tuple(silent) != tuple(c["skipped"]):
                fails.append(f"(d) subset: {tag}: the script's masks silence {silent}, not {c['skipped']}")
            if o["stats"] != (c["B"], len(silent)):
                fails.append(f"(d) subset: {tag}: skip counters advanced by {o['stats']}, expected {(c['B'], len(silent))}")
            if bias is not None:
                for b in silent:
                    if not np.array_equal(_bits(o["emb"][b]), _bits(np.broadcast_to(bias, o["emb"][b].shape).astype(np.float32))):
                        fails.append(f"(d) subset: {tag}: silent window {b} is not seg_1.bias")
        # (c) parity against float64
        ref = _window_rows(reference(script, c), skip)
        if c["kind"] == "seg":
            got, ml = _window_rows(o["logp"], skip), _window_rows(o["ml"], skip)
            if got.shape != ref.shape:
                fails.append(f"(c) parity: {tag}: shape {got.shape} against {ref.shape}")
                continue
            err = float(np.abs(got.astype(np.float64) - ref).max()) if np.isfinite(got).all() else float("inf")
            top = np.sort(ref, axis=-1)
            keep = (top[..., -1] - top[..., -2]) >= MARGIN
            agree_all = got.argmax(-1) == ref.argmax(-1)
            frames = int(keep.size)
            worst["dlogp"] = max(worst["dlogp"], err)
            worst["excluded"] += int((~keep).sum())
            worst["frames"] += frames
            if err > bar_logp:
                fails.append(f"(c) parity: {tag}: max |d logp| = {err:.3e} > {bar_logp}")
            if precision == "f16":
                share = float(agree_all[keep].mean()) if keep.any() else 1.0
                if frames >= F16_WAIVE_FRAMES:
                    worst["agree"] = min(worst["agree"], share)
                if frames >= F16_WAIVE_FRAMES and share < bar_agree:
                    fails.append(f"(c) parity: {tag}: argmax agreement {share:.4f} < {bar_agree} over {frames} frames")
            else:
                exp_ml = seg_model.to_multilabel(torch.from_numpy(ref), cfg).numpy().astype(np.uint8)
                if not agree_all[keep].all() or not np.array_equal(ml[keep], exp_ml[keep]):
                    fails.append(f"(c) parity: {tag}: {int((~agree_all[keep]).sum())} decisions differ from float64 outside near ties")
        else:
            got = _window_rows(o["emb"], skip).astype(np.float64).reshape(-1, 256)
            r = ref.reshape(-1, 256)
            cos = (got * r).sum(-1) / (np.linalg.norm(got, axis=-1) * np.linalg.norm(r, axis=-1))
            cmin = float(cos.min()) if np.isfinite(cos).all() else float("-inf")
            worst["cos"] = min(worst["cos"], cmin)
            if cmin < bar_cos:
                fails.append(f"(c) parity: {tag}: min cosine {cmin:.7f} < {bar_cos}")
    if worst["frames"] and worst["excluded"] > MAX_EXCLUDED * worst["frames"]:
        fails.append(f"(c) parity: {worst['excluded']} of {worst['frames']} frames are near ties of the reference (> {MAX_EXCLUDED:.0%}): change the seed")
    line = f"[engine reuse] {script['name']} {script['config']} {precision}: {len(calls)} calls"
    if worst["frames"]:
        line += f", worst max|dlogp| {worst['dlogp']:.2e}, near ties excluded {worst['excluded']}/{worst['frames']}"
        if precision == "f16":
            line += f", worst argmax agreement {worst['agree']:.4f}"
    else:
        line += f", worst min cosine {worst['cos']:.7f}"
    print(line + (f" -- {len(fails)} contract lines missed" if fails else ""))
    assert not fails, "\n".join(fails)
    return worst


# ------------------------------------------------------------------ a CPU model of a handle
MUTANTS = ("table_unkeyed", "pad_rows_stale", "tracker_not_reset", "border_not_rezeroed", "stride_by_B", "batch_global_max")


class ModelError(Exception):
    pass


class ModelEngine:
    """The float32 oracle behind the engine's interface, keeping state the way a handle does: flat workspaces sized for
    (max_batch, max_samples), zeroed ONCE and laid out per call by that call's geometry; tables cached by their key;
    |max| trackers strided by max_batch, reset per call, from which a per-window operand step is taken (the model's
    stand-in for the two-term split: the projected rows are rounded to 2^-21 of their window's |max|).  `mutant` breaks
    one line of that book-keeping (MUTANTS)."""
    AM_FEAT, AM_X, AM_COUNT = 0, 1, 2

    def __init__(self, cfg, sd, esd, max_batch, max_samples, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.cfg, self.sd, self.esd, self.mutant = cfg, sd, esd, mutant
        self.max_batch, self.max_samples = max_batch, max_samples
        self.maxL = seg_frames(cfg, max_samples)
        self.amax = torch.zeros(self.AM_COUNT * max_batch)
        self.xpad = torch.zeros(max_batch * (self.maxL + cfg.pos_conv_kernel) * cfg.embed_dim)
        self.table = torch.zeros(cfg.total_heads * (2 * self.maxL - 1))
        self.table_L = None
        self.maxT = emb_frames(max_samples)
        self.img = torch.zeros(max_batch * 82 * (self.maxT + 2)) if esd is not None else None
        self.emb_T, self.geoms = None, set()
        self.windows = self.skipped = 0

    def close(self):
        pass

    def skip_stats(self):
        return self.windows, self.skipped

    # ---- segmentation
    def _ensure_table(self, L):
        if L == self.table_L or (self.mutant == "table_unkeyed" and self.table_L is not None):
            return
        from oracle import seg_model as sm
        cfg = self.cfg
        bucket = sm.relpos_bucket(torch.arange(-(L - 1), L), cfg.num_buckets, cfg.max_distance)
        emb = self.sd[f"{sm.P}encoder.transformer.layers.0.attention.rel_attn_embed.weight"]
        self.table[:cfg.total_heads * (2 * L - 1)].view(cfg.total_heads, 2 * L - 1).copy_(emb[bucket].T)
        self.table_L = L

    @torch.inference_mode()
    def segment(self, wave):
        from oracle import seg_model as sm
        cfg, sd, MB = self.cfg, self.sd, self.max_batch
        B, N = wave.shape
        if B > MB or N > self.max_samples:
            raise ModelError("bad B / N")
        P, tp, D = sm.P, sm.P + "encoder.transformer", cfg.embed_dim
        if self.mutant != "tracker_not_reset":
            self.amax.zero_()
        feats = sm.feature_extractor(sd, cfg, wave)
        L = feats.shape[1]
        x = F.layer_norm(feats, (feats.shape[-1],), sd[P + "encoder.feature_projection.layer_norm.weight"],
                         sd[P + "encoder.feature_projection.layer_norm.bias"])
        x = F.linear(x, sd[P + "encoder.feature_projection.projection.weight"], sd[P + "encoder.feature_projection.projection.bias"])
        # producers write their window's |max| at slot * max_batch + b ...
        for b in range(B):
            for slot, t in ((self.AM_FEAT, feats), (self.AM_X, x)):
                m = (t if self.mutant == "batch_global_max" else t[b]).abs().max()
                self.amax[slot * MB + b] = torch.maximum(self.amax[slot * MB + b], m)
        # ... and the consumer takes its operand step from there
        stride = B if self.mutant == "stride_by_B" else MB
        x = x.clone()
        for b in range(B):
            step = self.amax[self.AM_X * stride + b] * 2.0 ** -21
            if step != 0:
                x[b] = torch.round(x[b] / step) * step
        # positional conv over the padded copy: window b at rows [b Lp, (b + 1) Lp), its L rows behind Kc/2 zero rows
        Kc, pad = cfg.pos_conv_kernel, cfg.pos_conv_kernel // 2
        Lp = L + Kc
        xp = self.xpad[:B * Lp * D].view(B, Lp, D)
        if self.mutant != "pad_rows_stale":
            xp[:, :pad] = 0.0
            xp[:, pad + L:] = 0.0
        xp[:, pad:pad + L] = x
        g_ = sd[tp + ".pos_conv_embed.conv.parametrizations.weight.original0"]
        v_ = sd[tp + ".pos_conv_embed.conv.parametrizations.weight.original1"]
        w = g_ * v_ / v_.norm(dim=(0, 1), keepdim=True)
        pc = F.conv1d(xp.transpose(1, 2), w, sd[tp + ".pos_conv_embed.conv.bias"], groups=cfg.pos_conv_groups)[..., :L]
        x = x + F.gelu(pc).transpose(1, 2)
        if not cfg.layer_norm_first:
            x = F.layer_norm(x, (D,), sd[tp + ".layer_norm.weight"], sd[tp + ".layer_norm.bias"])
        self._ensure_table(L)
        idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + (L - 1)
        pbias = self.table[:cfg.total_heads * (2 * L - 1)].view(cfg.total_heads, 2 * L - 1)[:, idx]
        reps = [x]
        for i in range(cfg.n_layers):            # oracle/seg_model.py:encoder, with this handle's table
            lp = f"{tp}.layers.{i}"
            ln1 = (sd[lp + ".layer_norm.weight"], sd[lp + ".layer_norm.bias"])
            ln2 = (sd[lp + ".final_layer_norm.weight"], sd[lp + ".final_layer_norm.bias"])

            def ffn(z):
                z = F.gelu(F.linear(z, sd[lp + ".feed_forward.intermediate_dense.weight"], sd[lp + ".feed_forward.intermediate_dense.bias"]))
                return F.linear(z, sd[lp + ".feed_forward.output_dense.weight"], sd[lp + ".feed_forward.output_dense.bias"])
            if cfg.remaining_heads[i]:
                y = F.layer_norm(x, (D,), *ln1) if cfg.layer_norm_first else x
                x = x + sm.wavlm_attention(sd, cfg, i, y, pbias)
            if cfg.layer_norm_first:
                x = x + ffn(F.layer_norm(x, (D,), *ln2))
            else:
                x = F.layer_norm(x, (D,), *ln1)
                x = x + ffn(x)
                x = F.layer_norm(x, (D,), *ln2)
            reps.append(x)
        z = torch.stack(reps, dim=-1) @ sd["weight_sum.weight"][0]
        z = F.layer_norm(F.linear(z, sd["proj.weight"], sd["proj.bias"]), (cfg.attention_in,), sd["lnorm.weight"], sd["lnorm.bias"])
        for i in range(cfg.conf_layers):
            z = sm.conformer_block(sd, cfg, i, z)
        logp = F.log_softmax(F.linear(z, sd["classifier.weight"], sd["classifier.bias"]), dim=-1)
        mapping = sm.powerset_mapping(cfg.max_speakers_per_chunk, cfg.max_speakers_per_frame)
        return {"logp": logp.numpy(), "ml": sm.to_multilabel(logp, cfg).to(torch.uint8).numpy(), "soft": (logp.exp() @ mapping).numpy()}

    # ---- embedding
    def _set_geometry(self, T):
        if T == self.emb_T:
            return
        if T not in self.geoms and len(self.geoms) >= MAX_GEOMS:
            raise ModelError("too many distinct window lengths on one handle")
        self.geoms.add(T)
        if self.mutant != "border_not_rezeroed":
            self.img.zero_()
        self.emb_T = T

    @torch.inference_mode()
    def embed(self, wave, masks, out=None):
        from oracle import emb_model as em
        esd, MB = self.esd, self.max_batch
        B, N = wave.shape
        T = emb_frames(N)
        if B > MB or T < 1 or T > self.maxT:
            raise ModelError("bad B / N")
        self._set_geometry(T)
        fb = em.compute_fbank(wave)
        active = [b for b in range(B) if bool(masks[b].any())]
        self.windows += B
        self.skipped += B - len(active)
        res = esd["resnet.seg_1.bias"].expand(B, masks.shape[1], -1).clone()
        if active:
            # the stem reads bordered images, pitch T + 2: only the interior is written, the border is zero since the geometry was set
            img = self.img[:MB * 82 * (T + 2)].view(MB, 82, T + 2)
            img[active, 1:81, 1:T + 1] = fb[active].permute(0, 2, 1)
            x = F.relu(em._bn(esd, "resnet.bn1", F.conv2d(img[active].unsqueeze(1), esd["resnet.conv1.weight"])))
            for s, nb in enumerate((3, 4, 6, 3)):        # oracle/emb_model.py:resnet_trunk behind the stem
                for j in range(nb):
                    p = f"resnet.layer{s + 1}.{j}"
                    stride = 2 if (j == 0 and s > 0) else 1
                    y = F.relu(em._bn(esd, p + ".bn1", F.conv2d(x, esd[p + ".conv1.weight"], stride=stride, padding=1)))
                    y = em._bn(esd, p + ".bn2", F.conv2d(y, esd[p + ".conv2.weight"], padding=1))
                    sc = em._bn(esd, p + ".shortcut.1", F.conv2d(x, esd[p + ".shortcut.0.weight"], stride=stride)) \
                        if (p + ".shortcut.0.weight") in esd else x
                    x = F.relu(y + sc)
            seq = x.reshape(len(active), x.shape[1] * x.shape[2], x.shape[3])
            res[active] = F.linear(em.stats_pool(seq, masks[active]), esd["resnet.seg_1.weight"], esd["resnet.seg_1.bias"])
        if out is not None:
            out.copy_(res)
        return res.numpy()

    def embed_strided(self, rec, B, N, stride, masks):
        return self.embed(rec.as_strided((B, N), (stride, 1)).contiguous(), masks)


def model_factory(config, with_emb, mutant=None):
    cfg = get_cfg(config)
    return lambda max_batch, max_samples: ModelEngine(cfg, seg_weights(config), emb_weights() if with_emb else None,
                                                      max_batch, max_samples, mutant)
