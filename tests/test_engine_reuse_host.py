"""CPU: the engine-reuse scripts of tests/_reuse_cases.py reach what they claim and their checks bite.  The shape tables,
derived from the configuration, hit every target; the float64 references are finite at every shape (L = 1 included), take
several classes and leave the near-tie exclusion far under its cap; a MODEL of a handle (the float32 oracle behind the
engine's interface, with flat workspaces zeroed once, tables cached by key and trackers strided by max_batch) passes
`check_script` on every script, and each of six one-line book-keeping mistakes in it misses the contract named for it.
The same scripts and the same `check_script` then judge the device handle in test_engine_reuse_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest

import _reuse_cases as rc

SEG_SCRIPTS = [("seg_history", c) for c in rc.SEG_CONFIGS] + [("poison_seg", c) for c in rc.SEG_CONFIGS]
EMB_SCRIPTS = ["emb_history", "emb_geometries", "poison_emb"]
_SCRIPTS = {}


def _script(name, config=rc.EMB_CONFIG):
    if (name, config) not in _SCRIPTS:
        _SCRIPTS[(name, config)] = {"seg_history": lambda: rc.seg_history(config), "poison_seg": lambda: rc.poison("seg", config),
                                    "emb_history": rc.emb_history, "emb_geometries": rc.emb_geometries,
                                    "poison_emb": lambda: rc.poison("emb", rc.EMB_CONFIG)}[name]()
    return _SCRIPTS[(name, config)]


def _bias():
    return rc.emb_weights()["resnet.seg_1.bias"].numpy()


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("config", rc.SEG_CONFIGS)
def test_segmentation_table_hits_every_target(config):
    cfg = rc.get_cfg(config)
    table = rc.seg_table(cfg)
    assert rc.seg_frames(cfg, rc.MAX_SAMPLES) == 49 == cfg.num_frames(rc.MAX_SAMPLES)
    assert all(1 <= B <= rc.MAX_BATCH and 400 <= N <= rc.MAX_SAMPLES for B, N in table)
    Ls = {rc.seg_frames(cfg, N) for _, N in table}
    rows = {B * rc.seg_frames(cfg, N) for B, N in table}
    assert set(rc.SEG_L_TARGETS) <= Ls
    assert {1, 2, 128, 129, 294} <= rows and (127 in rows or 126 in rows)
    assert {1, rc.MAX_BATCH} <= {B for B, _ in table}
    # smallest N: one sample less is one frame less
    assert all(N == rc.MAX_SAMPLES or rc.seg_frames(cfg, N - 1) == rc.seg_frames(cfg, N) - 1 for _, N in table)
    # the frame counts the issue was written with
    assert [rc.seg_frames(cfg, N) for N in (400, 720, 1520, 16000)] == [1, 2, 4, 49]
    print(f"\n[engine reuse] {config} segmentation table (B, N, L): " + " ".join(f"({B},{N},{rc.seg_frames(cfg, N)})" for B, N in table))


def test_embedding_table_hits_every_target():
    cfg = rc.get_cfg(rc.EMB_CONFIG)
    table = rc.emb_table()
    assert [rc.emb_frames(N) for _, N in table] == list(rc.EMB_T_TARGETS) and rc.emb_frames(1520) == 8
    assert {B for B, _ in table} == set(rc.EMB_B_TARGETS)
    assert all(N <= rc.MAX_SAMPLES and rc.emb_frames(N - 1) == rc.emb_frames(N) - 1 for _, N in table)
    widths = []
    for _, N in table:
        w, ws = rc.emb_frames(N), []
        for s in range(4):
            w = w if s == 0 else (w - 1) // 2 + 1
            ws.append(w)
        widths.append(tuple(ws))
    assert widths == [(8, 4, 2, 1), (9, 5, 3, 2), (17, 9, 5, 3), (98, 49, 25, 13)]
    for name in EMB_SCRIPTS:
        for c in _script(name)["calls"]:
            assert c["B"] <= rc.MAX_BATCH and c["N"] <= rc.MAX_SAMPLES
            assert c["masks"].shape == (c["B"], rc.S_MASKS, rc.seg_frames(cfg, c["N"]))
            assert set(np.unique(c["masks"].numpy()).tolist()) <= {0.0, 1.0}
    geo = _script("emb_geometries")["calls"]
    Ts = [rc.emb_frames(c["N"]) for c in geo]
    assert Ts[:rc.MAX_GEOMS] == list(range(8, 72)) and Ts[rc.MAX_GEOMS] == 72 and Ts[rc.MAX_GEOMS + 1:] == [8, 71]
    leg_b = [c for c in _script("emb_history")["calls"] if c["key"] == ("leg_b",)]
    assert len(leg_b) == 1 and [b for b in range(6) if not leg_b[0]["masks"][b].any()] == [1, 4]
    strided = [c for c in _script("emb_history")["calls"] if c["kind"] == "emb_strided"][0]
    assert strided["stride"] % 160 == 0 and strided["stride"] <= strided["N"] - 400 + 160          # the shared frame grid
    assert strided["rec"].numel() == (strided["B"] - 1) * strided["stride"] + strided["N"]


@pytest.mark.parametrize("name,config", SEG_SCRIPTS)
def test_segmentation_references_are_finite_varied_and_rarely_tied(name, config):
    script = _script(name, config)
    for c in script["calls"]:
        ref = rc.reference(script, c)
        keep = np.delete(ref, c["poisoned"], axis=0) if "poisoned" in c else ref
        assert np.isfinite(keep).all(), (c["B"], c["N"], c["phase"])
        assert ref.shape[:2] == (c["B"], rc.seg_frames(rc.get_cfg(config), c["N"]))
    low, total, classes = rc.margin_stats(script)
    print(f"\n[engine reuse] {name} {config}: {low} of {total} float64 frames have a top-2 margin under {rc.MARGIN}; classes {sorted(classes)}")
    assert low <= rc.MAX_EXCLUDED * total
    assert len(classes) >= 3


@pytest.mark.parametrize("name", EMB_SCRIPTS)
def test_embedding_references_are_finite(name):
    script = _script(name)
    for c in script["calls"]:
        ref = rc.reference(script, c)
        if ref is not None:
            assert np.isfinite(ref).all() and ref.shape == (c["B"], rc.S_MASKS, 256)


# ------------------------------------------------------------------ the model of a handle, and its six mistakes
_MODEL_RUNS = {}


def _run(name, config, mutant=None):
    with_emb = not name.endswith("seg") and name != "seg_history"
    script = _script(name, config)
    fit_cache = _MODEL_RUNS.setdefault(("fit", config, with_emb), {}) if mutant is None else {}
    return script, rc.run_script(rc.model_factory(config, with_emb, mutant), script, fit_cache)


@pytest.mark.parametrize("name,config", SEG_SCRIPTS + [(n, rc.EMB_CONFIG) for n in EMB_SCRIPTS])
def test_the_unmutated_model_passes_every_script(name, config):
    script, result = _run(name, config)
    worst = rc.check_script(script, result, "f32", bias=_bias(), error_type=rc.ModelError)
    assert worst["dlogp"] <= 1e-3 and worst["cos"] >= 0.9999


# mutant -> (script, configuration, the contract it must miss)
EXPECTED = {
    "table_unkeyed": ("seg_history", "tiny_ln", "(b) size"),            # both passes read the first L's table: only another handle shows it
    "pad_rows_stale": ("seg_history", "tiny_ln", "(a) history"),        # a previous longer call shows through the padding rows
    "tracker_not_reset": ("seg_history", "tiny_gn", "(a) history"),     # the gain-1e4 call's |max| survives into the second pass
    "border_not_rezeroed": ("emb_history", "tiny_ln", "(b) size"),      # the previous geometry's pixels sit in this one's borders
    "stride_by_B": ("seg_history", "tiny_ln", "(b) size"),              # the r4 class: invisible where max_batch == B
    "batch_global_max": ("poison_seg", "tiny_gn", "(f) isolation"),     # one non-finite window takes the batch's scale with it
}


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_each_mutant_misses_its_contract(mutant):
    name, config, contract = EXPECTED[mutant]
    script, result = _run(name, config, mutant)
    with pytest.raises(AssertionError) as e:
        rc.check_script(script, result, "f32", bias=_bias(), error_type=rc.ModelError)
    lines = str(e.value).splitlines()
    print(f"\n[engine reuse] mutant {mutant}: {len(lines)} contract lines missed on {name} {config}, first: {lines[0][:110]}")
    assert any(line.startswith(contract) for line in lines), str(e.value)


def test_stride_by_B_is_invisible_on_exact_fit_handles():
    """the reason this file exists: a handle created at exactly (B, N), as nearly every older engine test creates it, runs
    the r4 class of mistake without a trace"""
    script = _script("seg_history", "tiny_ln")
    good, bad = rc.model_factory("tiny_ln", False), rc.model_factory("tiny_ln", False, "stride_by_B")
    for c in script["calls"][:4]:
        a, b = good(c["B"], c["N"]).segment(c["wave"]), bad(c["B"], c["N"]).segment(c["wave"])
        assert all(np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)) for n in ("logp", "ml", "soft"))
