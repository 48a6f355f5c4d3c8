"""Kernel-level matrix of the contraction families (gemm.hip, gemm_split.hip, gemm_split_pre.hip, gemm_mx.hip): every tile,
forced by name and confirmed through the profiler class, crossed with the epilogue features, at shapes that put the tile edges
where the indexing is decided.  tests/_gemm_cases.py holds the shapes, inputs, float64 reference and the DERIVED per-element
bound (test_gemm_bounds_host.py shows on the CPU that an ideal kernel keeps a factor 4 under it).

Per launch: (1) every output element within its own bound of the float64 reference — per element, never against the global
maximum; (2) every buffer sits inside a larger allocation whose bands are compared bit for bit afterwards (inputs: NaN bands, so
a read outside the logical operand poisons the result; outputs: a fixed NaN bit pattern, so a store outside the logical output
changes a band and an element nobody stored is not finite); (3) every stored element finite; (4) c_amax[u] == max |C[rows of unit
u, :N]| of the STORED C, bit for bit, its guard entries still 0.0; (5) row statistics against float64 mean / rsqrt(var + eps) of
the stored C, per row; (6) a second identical launch gives the same bits everywhere.

E2's strides: ldc = N + 5 with N = 2 BN - 13 (a multiple of 4 — what takes the scalar epilogue there is N % 4 != 0), ldws = N + 6
(odd).  The worst error / bound ratio per (family, tile, feature) goes to gemm_tile_matrix.json, beside the report of
test_f32h_grade_gpu.py (DZN_REPORT_DIR overrides the directory).
"""
import json
import os
import re

import pytest
import torch

import _gemm_cases as gc

pytestmark = pytest.mark.gpu

G = gc.GUARD_ROWS
_REPORT = {}


def _report_dir():
    """the suite's report directory: where test_f32h_grade_gpu.py writes its report, so that this one lands beside it"""
    if os.environ.get("DZN_REPORT_DIR"):
        return os.environ["DZN_REPORT_DIR"]
    src = open(os.path.join(os.path.dirname(__file__), "test_f32h_grade_gpu.py")).read()
    return re.search(r'os\.makedirs\("([^"]+)"', src).group(1)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if _REPORT:
        out = _report_dir()
        os.makedirs(out, exist_ok=True)
        fam = {}
        for k, v in _REPORT.items():
            f = k.split("/")[0]
            fam[f] = max(fam.get(f, 0.0), v)
        json.dump({"worst_ratio_per_family": fam, "worst_ratio": _REPORT,
                   "note": "max over elements of |kernel - float64 reference| / derived bound (tests/_gemm_cases.py); > 1 fails"},
                  open(os.path.join(out, "gemm_tile_matrix.json"), "w"), indent=1)


def _in_buf(dev, total, idx, data, fill=float("nan"), dtype=torch.float32):
    buf = torch.full((total,), fill, dtype=dtype)
    buf[idx.reshape(-1)] = data.reshape(-1).to(dtype)
    return buf.to(dev)


def _out_buf(dev, total):
    return torch.full((total,), gc.PATTERN, dtype=torch.int32, device=dev)


def _read(buf, idx, what, ld, problems):
    """(stored values at idx as fp32, the raw host copy); notes a band that changed"""
    h = buf.cpu()
    vals = h[idx].view(torch.float32)
    band = h.clone()
    band[idx.reshape(-1)] = gc.PATTERN
    bad = (band != gc.PATTERN).nonzero().reshape(-1)
    if bad.numel():
        first = int(bad[0])
        problems.append(f"{what}: {bad.numel()} band elements changed, first at flat {first} = row {first // ld - G}, col {first % ld} "
                        f"(rows counted from the logical origin, ld {ld})")
    return vals, h


def _profiled(**kw):
    from diarizen_amd import _lib, ops
    _lib.profile_enable(True)
    try:
        out = ops.gemm(**kw)
        names = [p["name"] for p in _lib.profile_collect() if p["name"].startswith("gemm_")]
    finally:
        _lib.profile_enable(False)
    return out, names


def _weights(dev, family, W, N, K):
    """W with NaN band rows before and after, split TOGETHER with its band; the per-row scales of the band poisoned too"""
    from diarizen_amd import ops
    full = torch.full((G + N + G, K), float("nan"))
    full[G:G + N] = W
    full = full.to(dev)
    kw = dict(W=full[G:], N=N, K=K, ldw=K)
    if family == "f32" or K % 32:
        return kw

    def poison(cs):
        cs = cs.clone()
        cs[:G] = float("nan")
        cs[G + N:] = float("nan")
        return cs[G:]
    kw["W3"] = ops.split_weights(full)[G:]
    if family in ("f32h", "f16", "mx"):
        w2, cs = ops.split_weights_h2(full)
        kw["W2h"], kw["col_scale"] = w2[G:], poison(cs)
    if family == "mx":
        wm, cm = ops.split_weights_mx(full)
        kw["Wmx"], kw["col_scale_mx"], kw["mx"] = wm[G:], poison(cm), True
    return kw


def _vec(dev, data, fill=float("nan"), dtype=torch.float32, pad=4):
    """a vector with `pad` band entries either side: (whole device buffer, the logical view)"""
    n = data.numel()
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype)
    buf[pad:pad + n] = data.to(dtype)
    buf = buf.to(dev)
    return buf, buf[pad:]


def run_case(dev, family, tile, M, N, K, fname, unit, *, odd=False, nz=1, zsel=None, g_layout=False, geom=None, want_stats=None,
             seed=0):
    """one launch (two for the layer-weighted sum) of `family` on an M x N x K problem with feature set `fname`, every buffer in
    bands; asserts 1-5 of the module docstring, records the worst error / bound, returns the raw host copies of every output"""
    from diarizen_amd import ops
    prec, tag, tiles = gc.FAMILIES[family]
    feat = gc.FEATURES[fname]
    BM, BN, WGM, WGN = geom or tiles[tile]       # geom: the automatic tile this launch is expected to take (tile = None)
    cls = f"gemm_{tag}_{BM}x{BN}"
    pre = family == "f32s_pre"
    inp = gc.make_inputs(M, N, K, unit, nz, seed)
    zs = list(range(nz)) if zsel is None else zsel
    problems = []
    coord = f"{family}/{tile or 'auto'} {M}x{N}x{K} nz={nz} {fname} unit={unit}"

    # ---- A ----
    lda = K if g_layout else K + (32 if pre else 8)
    a_z0 = M * K if g_layout else (M + 16) * lda
    g = torch.Generator().manual_seed(M + N)
    arow = torch.randperm(M, generator=g) if feat.get("rowoff") else torch.arange(M)
    crow = torch.randperm(M, generator=g) if feat.get("rowoff") else torch.arange(M)
    baseA = G * lda
    idxA = baseA + (torch.arange(nz) * a_z0)[:, None, None] + (arow * lda)[None, :, None] + torch.arange(K)[None, None, :]
    totA = (baseA + nz * a_z0 + G * lda + lda - 1) // lda * lda
    Abuf = _in_buf(dev, totA, idxA, inp["A"])
    kw = dict(A=Abuf[baseA:], M=M, lda=lda, precision=prec, nz=nz)
    if pre:
        planes = ops.split_rows(Abuf.view(-1, lda))
        kw["a_planes"] = planes[:, G:, :]
    kw.update(_weights(dev, family, inp["W"], N, K))
    keep = [Abuf]

    # ---- C, R, WS ----
    ldc = N + (5 if odd else 8)
    ldws = N + (6 if odd else 8)
    c_z0 = (M + 16) * ldc
    baseC = G * ldc
    totC = baseC + nz * c_z0 + G * ldc
    idxC = baseC + (torch.tensor(zs) * c_z0)[:, None, None] + (crow * ldc)[None, :, None] + torch.arange(N)[None, None, :]
    Cbuf = _out_buf(dev, totC)
    kw.update(C_out=Cbuf.view(torch.float32)[baseC:], ldc=ldc)
    zsd = dict(a_z0=a_z0, c_z0=c_z0) if nz > 1 else {}
    if zsel is not None:
        zl = torch.tensor(zs + [1] * (nz - len(zs)), dtype=torch.int32, device=dev)
        zc = torch.tensor([len(zs)], dtype=torch.int32, device=dev)
        keep += [zl, zc]
        zsd.update(z_list=zl.data_ptr(), z_count=zc.data_ptr())
    kw["zs"] = zsd
    if feat.get("rowoff"):
        abuf, aoff = _vec(dev, arow * lda, fill=-lda, dtype=torch.int32)
        cbuf, coff = _vec(dev, crow * ldc, fill=-ldc, dtype=torch.int32)
        keep += [abuf, cbuf]
        kw.update(a_rowoff=aoff, c_rowoff=coff)
    if feat.get("R"):
        idxR = baseC + (torch.arange(nz) * c_z0)[:, None, None] + (crow * ldc)[None, :, None] + torch.arange(N)[None, None, :]
        Rbuf = _in_buf(dev, totC, idxR, inp["R"])
        keep.append(Rbuf)
        kw["R"] = Rbuf[baseC:]
    bbuf, bias = _vec(dev, inp["bias"])
    keep.append(bbuf)
    kw.update(bias=bias, act=feat.get("act", 0), alpha=feat.get("alpha", 1.0), post_relu=feat.get("post_relu", False))

    # ---- |max| trackers: a_amax in, c_amax out (guards 0.0: a sentinel above every float would hide an atomicMax) ----
    nu = gc.n_units(M, unit, nz)
    abuf2, a_amax = _vec(dev, inp["a_amax"], fill=gc.A_AMAX_GUARD)
    cabuf, c_amax = _vec(dev, torch.zeros(nu), fill=0.0)
    keep.append(abuf2)
    kw.update(a_amax=a_amax, c_amax=c_amax, amax_unit=unit, amax_guard=4)

    # ---- folded LayerNorm in, row statistics out ----
    ln = None
    if feat.get("ln"):
        st = ops.row_stats(inp["A"][0].to(dev), K, 1e-5).cpu()
        cs = inp["W"].double().sum(1).float()
        ln = (st[:, 0].contiguous(), st[:, 1].contiguous(), cs)
        lbuf, lstats = _vec(dev, st.reshape(-1), pad=2 * G)
        cbuf2, lcs = _vec(dev, cs)
        keep += [lbuf, cbuf2]
        kw.update(ln_stats=lstats, ln_colsum=lcs)
    stats = feat.get("stats", False) if want_stats is None else want_stats
    if stats:
        tilesN = (N + BN - 1) // BN
        P, pmax = tilesN * WGN, 2 * ((N + 63) // 64)
        pband = 2 * pmax * G
        Pbuf, Fbuf = _out_buf(dev, M * pmax * 2 + 2 * pband), _out_buf(dev, M * 2 + 4 * G)
        kw.update(want_row_stats=True, stat_bufs=(Pbuf.view(torch.float32)[pband:], Fbuf.view(torch.float32)[2 * G:]))

    # ---- launch ----
    WSbuf = None
    if feat.get("ws"):
        totW = G * ldws + (M + G) * ldws
        WSbuf = _out_buf(dev, totW)
        for w, init in zip(gc.WS_W, (True, False)):
            _, names = _profiled(**kw, WS=WSbuf.view(torch.float32)[G * ldws:], ldws=ldws, ws_w=w, ws_init=init)
            assert names == [cls], (coord, names, cls)
    else:
        _, names = _profiled(**kw, ldws=ldws)
        assert names == [cls], (coord, names, cls)
    torch.cuda.synchronize()

    # ---- read back and check ----
    raw = {}
    Cv, raw["C"] = _read(Cbuf, idxC, "C", ldc, problems)
    refs = [gc.launch_ref(family, inp, z, feat, ln) for z in zs]
    worst = 0.0

    def compare(name, got, want, bound):
        nonlocal worst
        if not torch.isfinite(got).all():
            bad = (~torch.isfinite(got)).nonzero()[0].tolist()
            problems.append(f"{name}: {int((~torch.isfinite(got)).sum())} stored elements not finite, first (z, m, n) = {bad}")
            return
        ratio = (got.double() - want).abs() / bound
        r = float(ratio.max())
        worst = max(worst, r)
        if not r <= 1.0:
            z, m, n = [int(v) for v in (ratio == ratio.max()).nonzero()[0]]
            problems.append(f"{name}: error / bound = {r:.3g} at (z, m, n) = ({z}, {m}, {n}): row {m % BM} of its row tile, column "
                            f"{n % BN} of its column tile; got {float(got[z, m, n])!r} want {float(want[z, m, n])!r}")
    compare("C", Cv, torch.stack([r["C"] for r in refs]), torch.stack([r["eC"] for r in refs]))
    if WSbuf is not None:
        idxW = G * ldws + torch.arange(M)[:, None] * ldws + torch.arange(N)[None, :]
        Wv, raw["WS"] = _read(WSbuf, idxW, "WS", ldws, problems)
        compare("WS", Wv[None], refs[0]["WS"][None], refs[0]["eWS"][None])
    # tracker: exact maximum of what was stored
    ca = cabuf.cpu()
    raw["c_amax"] = ca
    want = torch.zeros(nu)
    ru = gc.row_units(M, unit, nz)[zs]
    if torch.isfinite(Cv).all():
        want.scatter_reduce_(0, ru.reshape(-1), Cv.abs().amax(-1).reshape(-1), "amax")
        if not torch.equal(ca[4:4 + nu].view(torch.int32), want.view(torch.int32)):
            u = int((ca[4:4 + nu] != want).nonzero()[0])
            problems.append(f"c_amax[{u}] = {float(ca[4 + u])!r}, the stored C of unit {u} has max |.| {float(want[u])!r}")
    if not (torch.equal(ca[:4].view(torch.int32), torch.zeros(4, dtype=torch.int32))
            and torch.equal(ca[4 + nu:].view(torch.int32), torch.zeros(4, dtype=torch.int32))):
        problems.append(f"c_amax guard entries changed: {ca[:4].tolist()} | {ca[4 + nu:].tolist()}")
    if stats:
        idxP = pband + torch.arange(M * P * 2)
        _, raw["stat_partial"] = _read(Pbuf, idxP, "stat_partial", 2 * P, problems)
        Fv, raw["stat_final"] = _read(Fbuf, 2 * G + torch.arange(M * 2).view(M, 2), "stat_final", 2, problems)
        Cd = Cv[0].double()
        mu, var = Cd.mean(1), Cd.var(1, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        if not torch.isfinite(Fv).all():
            problems.append("stat_final: elements not finite")
        else:
            # test_gemm_mx_layernorm_folded_and_row_stats's two bounds (1e-4), per row: the mean against the row's mean |C|
            emu_, ers = (Fv[:, 0].double() - mu).abs() / Cd.abs().mean(1).clamp_min(1e-30), (Fv[:, 1].double() - rstd).abs() / rstd
            if not (float(emu_.max()) < 1e-4 and float(ers.max()) < 1e-4):
                problems.append(f"row statistics: mean off by {float(emu_.max()):.3g} of mean |C| (row {int(emu_.argmax())}), rstd by "
                                f"{float(ers.max()):.3g} relative (row {int(ers.argmax())})")
    key = f"{family}/{tile or 'auto'}/{fname}"
    _REPORT[key] = max(_REPORT.get(key, 0.0), worst)
    assert not problems, coord + "\n" + "\n".join(problems)
    return raw


def run_twice(*a, **kw):
    """assertion 6: the same launch again gives the same bits in every output (gemm_epilogue.h: fixed reduction order)"""
    r1, r2 = run_case(*a, **kw), run_case(*a, **kw)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), (a, kw, f"{k} differs between two identical launches")


def _forced(family, tile):
    from diarizen_amd import _lib
    lib = _lib.load()
    return lib.dzn_op_set_gemm_mx_cfg if family == "mx" else lib.dzn_op_set_gemm_cfg


@pytest.mark.parametrize("family,tile", gc.FAMILY_TILES)
def test_tile_edges_and_epilogue_features(built_lib, gpu, family, tile):
    """one tile of one family, forced by name (the profiler class must carry it), on the edge shapes E1-E4 crossed with the feature
    sets F0-F4; scale units of 24, TM and 99 rows reach the three tracker branches and put unit boundaries at odd rows inside
    wavefront tiles; the plain family also at K = 40 / 104 (register-staged kernel), MX at K = 64 / 96 / 128 / 544"""
    from diarizen_amd import _lib
    BM, BN, WGM, WGN = gc.FAMILIES[family][2][tile]
    TM = BM // WGM
    sh = gc.edge_shapes(BM, BN, mx=family == "mx")
    pre = family == "f32s_pre"
    setter = _forced(family, tile)
    setter(tile.encode())
    try:
        for e, feats in (("E1", ["F0", "F1", "F2", "F3", "F4"]), ("E2", ["F0", "F1", "F2", "F3"]), ("E3", ["F0", "F3"]),
                         ("E4a", ["F0"]), ("E4b", ["F0"]), ("E4c", ["F0"])):
            M, N, K, odd = sh[e]
            for f in feats:
                units = [24, TM, 99] if f == "F3" else [{"F0": 99, "F1": 24, "F2": TM, "F4": 24}[f]]
                for unit in units:
                    if f == "F3" and pre:
                        # row statistics are not finalized for the pre-split family: refused, then F3 without them
                        with pytest.raises(_lib.DznError, match="invalid argument"):
                            run_case(gpu, family, tile, M, N, K, f, unit, odd=odd)
                        run_twice(gpu, family, tile, M, N, K, f, unit, odd=odd, want_stats=False)
                    else:
                        run_twice(gpu, family, tile, M, N, K, f, unit, odd=odd)
        M, N, _, _ = sh["E1"]
        M2, N2, _, _ = sh["E2"]
        if family == "f32":
            run_twice(gpu, family, tile, M, N, 40, "F0", 99)
            run_twice(gpu, family, tile, M, N, 40, "F1", 24)
            run_twice(gpu, family, tile, M, N, 104, "F3", TM)
            run_twice(gpu, family, tile, M2, N2, 104, "F0", 99, odd=True)
        if family == "mx":
            run_twice(gpu, family, tile, M, N, 128, "F0", 99)
    finally:
        setter(b"auto")


@pytest.mark.parametrize("N,BN", gc.PLAIN_AUTO_WIDTHS)
def test_plain_automatic_column_tiles(built_lib, gpu, N, BN):
    """the 128 x 192 / 160 / 96 tiles launch_f32 picks by padded width (K = 544 > 512): partial last column tile, partial second
    row tile, with the residual epilogue, the folded LayerNorm + statistics + trackers, and the scalar epilogue at N - 1"""
    assert gc.auto_tile_f32(N, 544) == (128, BN) and gc.auto_tile_f32(N - 1, 544) == (128, BN)
    for f, unit, n, odd in (("F0", 99, N, False), ("F1", 24, N, False), ("F3", 64, N, False), ("F3", 99, N - 1, True)):
        run_twice(gpu, "f32", None, 145, n, 544, f, unit, odd=odd, geom=(128, BN, 2, 2))


@pytest.mark.parametrize("family", list(gc.FAMILIES))
def test_device_chosen_batch_subset(built_lib, gpu, family):
    """F5: nz = 5 with z_list = [3, 0, 4], z_count = [3]: the three listed slabs are right (per-z scale units: a_amax[z0] and
    c_amax[z0] follow the LISTED index), the two unlisted slabs and their trackers keep their bits"""
    tile = next(iter(gc.FAMILIES[family][2]))
    BM, BN = gc.FAMILIES[family][2][tile][:2]
    setter = _forced(family, tile)
    setter(tile.encode())
    try:
        run_twice(gpu, family, tile, BM + 17, 2 * BN - 12, 96, "F0", 0, nz=5, zsel=[3, 0, 4])
    finally:
        setter(b"auto")


G_GEOM = {"f32s": (128, 128, 2, 2), "f32h": (128, 128, 4, 1), "f16": (256, 128, 8, 1)}


@pytest.mark.parametrize("family", ["f32s", "f32h", "f16"])
@pytest.mark.parametrize("N", [244, 160])
def test_large_grid_automatic_wide_tiles(built_lib, gpu, family, N):
    """G1-G4: 273 x N x 544, nz = 75 with shared weights reaches the 448 workgroups behind which launch_gemm_split_np takes the
    wide tile (N = 244: 128 x 128, 256 x 128 for f16) or the exact 128 x 80 tile (N = 160); a guard slab between the z outputs,
    one scale unit per z"""
    M, K, nz = 273, 544, 75
    geom = G_GEOM[family] if N == 244 else (128, 80, 4, 1)
    assert gc.auto_tile_split(family, M, N, K, nz) == geom[:2]
    run_twice(gpu, family, None, M, N, K, "F0", 0, geom=geom, nz=nz, g_layout=True)


def test_large_grid_automatic_mx_wide_tile(built_lib, gpu):
    """G5: the MX family's automatic 128 x 128 tile (K = 96, nz = 75)"""
    assert gc.auto_tile_mx(273, 244, 75) == (128, 128)
    run_twice(gpu, "mx", None, 273, 244, 96, "F0", 0, geom=(128, 128, 4, 1), nz=75, g_layout=True)


def test_large_grid_kv_planes_on_the_wide_tile(built_lib, gpu):
    """G6: K / V planes are refused under a forced tile, so the wide tile writes them only at a grid of >= 448 workgroups:
    9517 x 768 x 544 (75 x 6 tiles of 128 x 128), kv_col0 = 256.  The fp32 columns against float64 at the f32h bound, the planes
    decoded as test_gemm_epilogue_writes_kv_planes decodes them, plane rows past M and the bands of the scale array untouched.
    Tracker rule (gemm_epilogue.h: the row maximum is taken over every existing column BEFORE a slot leaves as planes): c_amax
    covers the plane columns too, so it equals, bit for bit, the maximum of the plain launch's stored C over all N columns."""
    from diarizen_amd import _lib, ops
    M, N, K, col0, unit = 9517, 768, 544, 256, 399
    assert gc.auto_tile_split("f32h", M, N, K, 1) == (128, 128)
    inp = gc.make_inputs(M, N, K, unit)
    nu = gc.n_units(M, unit)
    A = inp["A"][0].to(gpu)
    wk = _weights(gpu, "f32h", inp["W"], N, K)
    bbuf, bias = _vec(gpu, inp["bias"])
    abuf, a_amax = _vec(gpu, inp["a_amax"], fill=gc.A_AMAX_GUARD)
    S = (N - col0) // 64
    out = {}
    for kv in (False, True):
        cabuf, c_amax = _vec(gpu, torch.zeros(nu), fill=0.0)
        kw = dict(A=A, bias=bias, precision=3, a_amax=a_amax, c_amax=c_amax, amax_unit=unit, amax_guard=4, **wk)
        if kv:
            planes = torch.full((2, M + 2 * G, N - col0), 0x5A5A, dtype=torch.int16, device=gpu)
            inv = torch.full(((M + 2 * G) * S,), -7.0, device=gpu)
            C = torch.full((M, N), float("nan"), device=gpu)
            (_, _, _), names = _profiled(**kw, C_out=C, kv_col0=col0, kv_bufs=(planes[:, G:, :], inv[G * S:]))
            out[kv] = (C, planes, inv.view(M + 2 * G, S), cabuf.cpu())
        else:
            C, names = _profiled(**kw)
            out[kv] = (C, cabuf.cpu())
        assert names == ["gemm_f32h_128x128"], names
    torch.cuda.synchronize()
    plain, ca_plain = out[False]
    C, planes, inv, ca = out[True]
    ref = gc.launch_ref("f32h", inp, 0, gc.FEATURES["F0"])
    ratio = ((plain.cpu().double() - ref["C"]).abs() / ref["eC"])
    _REPORT["f32h/auto128x128/kv"] = float(ratio.max())
    assert float(ratio.max()) <= 1.0, ratio.max()
    assert torch.equal(C[:, :col0], plain[:, :col0]) and torch.isnan(C[:, col0:]).all()     # the slots left as planes, only
    hi, lo = planes[0, G:G + M].view(torch.float16).float(), planes[1, G:G + M].view(torch.float16).float()
    rec = ((hi + lo).view(M, S, 64) * inv[G:G + M, :, None]).view(M, N - col0)
    want = plain[:, col0:]
    slot_max = want.view(M, S, 64).abs().amax(-1, keepdim=True)
    assert float(((rec - want).view(M, S, 64).abs() / slot_max.clamp_min(1e-30)).max()) <= 2.0 ** -21
    scaled = hi.view(M, S, 64).abs().amax(-1)
    assert float(scaled.min()) >= 2.0 ** 14 - 8 and float(scaled.max()) < 2.0 ** 15 + 1
    band = torch.cat([planes[:, :G], planes[:, G + M:]], 1)
    assert torch.equal(band, torch.full_like(band, 0x5A5A)), "plane rows outside [0, M) were written"
    assert torch.equal(inv[:G], torch.full_like(inv[:G], -7.0)) and torch.equal(inv[G + M:], torch.full_like(inv[G + M:], -7.0))
    want_ca = torch.zeros(nu)
    want_ca.scatter_reduce_(0, gc.row_units(M, unit)[0], plain.cpu().abs().amax(-1), "amax")
    for t in (ca_plain, ca):
        assert torch.equal(t[4:4 + nu].view(torch.int32), want_ca.view(torch.int32))
        assert not t[:4].any() and not t[4 + nu:].any()


def test_row_stats_scratch_is_sized_before_the_launch(built_lib, gpu):
    """ops.gemm's own statistics scratch holds 32 partials per row: a width that could leave more is refused before any launch"""
    from diarizen_amd import ops
    A, W = torch.zeros(8, 32, device=gpu), torch.zeros(1056, 32, device=gpu)
    with pytest.raises(ValueError, match="partials per row"):
        ops.gemm(A, W, want_row_stats=True)
