"""CPU check of the bounds test_gemm_tiles_gpu.py holds the contraction kernels to (tests/_gemm_cases.py): on the exact inputs of
the matrix an IDEAL kernel — the family's operand rounding emulated in float64 (testkit/mx_emulation.py), fp32 accumulation with
one rounding per step in two different orders (forward over k; blocked by 32, then by 4), an fp32 epilogue — stays at least a
factor 4 inside every bound.  So a ratio above 1 on the device is the kernel's, not the derivation's.  The factor is asked of
the share of a bound that descends from the accumulation (bound_acc: everything a kernel's order of operations can move); the
epilogue's own roundings are single operations whose error no kernel can exceed and an ideal one can reach (an element that is
all residual is rounded once, to u |y| exactly), so they enter at their face value: |error| <= bound_acc / 4 + bound_rounding.
Also here: the input conditions the bounds rely on, and the automatic tile rules the large-grid and column-tile cases of the
matrix claim.

The large-grid inputs are checked on a subset (z = 0, 1, 2 and the last z; the first and last 128 rows of the 9517-row case):
the scale units cycle through three loudness values, so these slabs cover every one of them with the same distribution.
"""
import pytest
import torch

import _gemm_cases as gc

ROOM = 4.0
ORDERS = ("forward", "blocked")


def _family_shapes(family):
    """the distinct (M, N, K, TM) the matrix runs for a family's tiles, with the features and units it runs on each"""
    out = {}
    for tile, (BM, BN, WGM, WGN) in gc.FAMILIES[family][2].items():
        TM = BM // WGM
        sh = gc.edge_shapes(BM, BN, mx=family == "mx")
        plan = [("E1", "F0", 99), ("E1", "F1", 24), ("E1", "F2", TM), ("E1", "F4", 24), ("E2", "F0", 99), ("E2", "F1", 24),
                ("E2", "F2", TM), ("E3", "F0", 99), ("E4a", "F0", 99), ("E4b", "F0", 99), ("E4c", "F0", 99)]
        plan += [(e, "F3", u) for e in ("E1", "E2", "E3") for u in (24, TM, 99)]
        for e, f, unit in plan:
            M, N, K, _ = sh[e]
            out.setdefault((M, N, K, unit), set()).add(f)
        M, N = sh["E1"][:2]
        if family == "f32":
            for K, f, unit in ((40, "F0", 99), (40, "F1", 24), (104, "F3", TM)):
                out.setdefault((M, N, K, unit), set()).add(f)
            out.setdefault((sh["E2"][0], sh["E2"][1], 104, 99), set()).add("F0")
        if family == "mx":
            out.setdefault((M, N, 128, 99), set()).add("F0")
    if family == "f32":
        for N, _ in gc.PLAIN_AUTO_WIDTHS:
            out.setdefault((145, N, 544, 99), set()).add("F0")
            out.setdefault((145, N, 544, 24), set()).add("F1")
            out.setdefault((145, N, 544, 64), set()).add("F3")
            out.setdefault((145, N - 1, 544, 99), set()).add("F3")
    return out


def _check(family, inp, z, feats, rows=None):
    """worst (ideal kernel error) / bound over the feature sets, both accumulation orders"""
    A, W, ra = inp["A"][z], inp["W"], inp["row_amax"][z]
    R = inp["R"][z]
    if rows is not None:
        A, ra, R = A[rows], ra[rows], R[rows]
    sub = dict(A=A[None], W=W, bias=inp["bias"], R=R[None], row_amax=ra[None])
    terms = gc.operand_terms(family, A, ra, W)
    worst = 0.0
    for order in ORDERS:
        acc = gc.ideal_accumulate(terms, order)
        for f in sorted(feats):
            feat = gc.FEATURES[f]
            ln = gc.host_ln(A, W, A.shape[1]) if feat.get("ln") else None
            ref = gc.launch_ref(family, sub, 0, feat, ln)
            got = gc.ideal_epilogue(acc, bias=inp["bias"], ln=ln, act=feat.get("act", 0), alpha=feat.get("alpha", 1.0),
                                    R=R if feat.get("R") else None, post_relu=feat.get("post_relu", False))
            r = float(((got.double() - ref["C"]).abs() / (ref["eC_acc"] / ROOM + (ref["eC"] - ref["eC_acc"]))).max())
            if feat.get("ws"):
                w1, w2 = (torch.tensor(w, dtype=torch.float32) for w in gc.WS_W)
                ws = w1 * got
                ws = ws + w2 * got
                r = max(r, float(((ws.double() - ref["WS"]).abs() / (ref["eWS_acc"] / ROOM + (ref["eWS"] - ref["eWS_acc"]))).max()))
            assert r <= 1.0, (family, tuple(A.shape), W.shape[0], f, order, r)
            worst = max(worst, r)
    return worst


@pytest.mark.parametrize("family", list(gc.FAMILIES))
def test_ideal_kernel_keeps_a_factor_4_under_every_bound_on_the_edge_inputs(family):
    worst = 0.0
    for (M, N, K, unit), feats in sorted(_family_shapes(family).items()):
        worst = max(worst, _check(family, gc.make_inputs(M, N, K, unit), 0, feats))
    print(f"[{family}] worst ideal-kernel error / (bound_acc / 4 + bound_rounding) on the edge inputs: {worst:.3f}")


@pytest.mark.parametrize("family,N,K", [("f32s", 244, 544), ("f32h", 244, 544), ("f16", 244, 544), ("f32s", 160, 544),
                                        ("f32h", 160, 544), ("f16", 160, 544), ("mx", 244, 96)])
def test_ideal_kernel_keeps_a_factor_4_under_the_bound_on_the_large_grid_inputs(family, N, K):
    inp = gc.make_inputs(273, N, K, 0, 75)
    for z in (0, 1, 2, 74):
        _check(family, inp, z, {"F0"})


def test_ideal_kernel_keeps_a_factor_4_under_the_bound_on_the_kv_plane_inputs():
    inp = gc.make_inputs(9517, 768, 544, 399)
    rows = torch.cat([torch.arange(128), torch.arange(9517 - 128, 9517)])
    _check("f32h", inp, 0, {"F0"}, rows=rows)


@pytest.mark.parametrize("M,N,K,unit,nz", [(145, 244, 96, 24, 1), (273, 243, 96, 99, 1), (255, 132, 544, 64, 1), (273, 244, 544, 0, 75),
                                           (17, 36, 32, 99, 1)])
def test_input_conditions_the_bounds_rely_on(M, N, K, unit, nz):
    """every element inside 2^10 of its unit maximum, a_amax the exact unit maximum, loudness 2^-9 / 1 / 2^7 by unit; hence no lo
    term of the fp16 split (activations per unit, weights per row) loses a bit to the subnormal grid: fp16(lo) keeps the full
    relative precision 2^-11 of every remainder"""
    inp = gc.make_inputs(M, N, K, unit, nz)
    A, ra = inp["A"], inp["row_amax"]
    assert torch.isfinite(A).all() and (A.abs() * 2.0 ** 10 >= ra).all() and (A.abs() <= ra).all()
    ru = gc.row_units(M, unit, nz)
    for u in range(gc.n_units(M, unit, nz)):
        m = float(A[ru == u].abs().max())
        assert m == float(inp["a_amax"][u]) and 2.0 ** -10 < m / [2.0 ** -9, 1.0, 2.0 ** 7][u % 3] <= 1.0
    W = inp["W"]
    wmax = W.abs().amax(1, keepdim=True)
    assert (W.abs() * 2.0 ** 11 >= wmax).all()
    for x, amax in ((A.reshape(-1, K), ra.reshape(-1, 1)), (W, wmax)):
        xs = (x.double() * gc.h2_row_scale(amax)).float()
        rem = xs - xs.to(torch.float16).float()
        lo = rem.to(torch.float16).float()
        assert ((rem - lo).abs() <= 2.0 ** -11 * rem.abs()).all()
        assert (xs.abs() < 2.0 ** 15).all() and (xs.abs() >= 2.0 ** 3).all()


def test_automatic_tile_rules_select_what_the_matrix_claims():
    """launch_f32 / launch_gemm_split_np / launch_gemm_mx restated: the large-grid cases reach the wide and the exact 80-wide
    tiles, the three plain widths their column tiles, and the shapes of the older kernel tests stay on the narrow tile"""
    for N, BN in gc.PLAIN_AUTO_WIDTHS:
        assert gc.auto_tile_f32(N, 544) == (128, BN) and gc.auto_tile_f32(N - 1, 544) == (128, BN)
    assert gc.auto_tile_f32(256, 512) == (128, 64) and gc.auto_tile_f32(20, 544) == (256, 32) and gc.auto_tile_f32(256, 544) == (128, 128)
    assert 3 * 2 * 75 >= 448
    for fam, want in (("f32s", (128, 128)), ("f32h", (128, 128)), ("f16", (256, 128))):
        assert gc.auto_tile_split(fam, 273, 244, 544, 75) == want
        assert gc.auto_tile_split(fam, 273, 160, 544, 75) == (128, 80)
        assert gc.auto_tile_split(fam, 273, 244, 544, 74) == (128, 64)      # 444 workgroups: still narrow
        assert gc.auto_tile_split(fam, 273, 244, 512, 75) == (128, 64)      # K <= 512: narrow whatever the grid
        assert gc.auto_tile_split(fam, 513, 1770, 1024) == (128, 64) and gc.auto_tile_split(fam, 1000, 3072, 1024) == (128, 64)
    assert gc.auto_tile_split("f32h", 9517, 768, 544) == (128, 128)
    assert gc.auto_tile_mx(273, 244, 75) == (128, 128) and gc.auto_tile_mx(273, 244, 74) == (128, 64)


def test_tile_table_lists_every_tile_the_issue_names():
    names = {f: set(t) for f, (_, _, t) in gc.FAMILIES.items()}
    assert names["f32"] == {"128x32", "256x32", "256x64", "128x64", "64x64", "128x128"}
    assert names["f32s"] == {"128x64", "128x80", "128x32", "128x128"}
    assert names["f32h"] == {"128x64", "128x80", "128x32", "128x128w4"}
    assert names["f16"] == names["f32h"] | {"256x128w8s3"}
    assert names["mx"] == {"128x64", "128x128", "256x128"} and names["f32s_pre"] == {"256x128", "128x128", "128x64"}
