"""Short-K contraction class (out_proj / FFN-down: N = 1024, K = 128 .. 512, residual epilogue + LayerNorm partials) per tile:
    python scripts/bench_gemm_small_tiles.py [--tiles auto,128x64,128x128w4,...] [--out table.txt]
walks every tile in one process (dzn_op_set_gemm_cfg) over M = 223 839, N = 1024, K = 128 .. 512 and the class's other wide
member N = 768, K = 256; 20 launches per row.  Per row: the profiler class the launch took, its device time from the in-situ
profiler (the contraction alone: the statistics finalize behind it is a class of its own), algorithmic TFLOP/s and TB/s, the
event time of the whole loop per launch (contraction + finalize), and the outputs against the FIRST tile of the list: C must be
bit-identical whatever the tile (every tile walks K in the same order); (mean, rstd) are sums over wavefront tiles of another
width, so they may move by roundings and the largest relative difference is printed instead."""
import argparse
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from diarizen_amd import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--tiles", default="auto,128x64,128x128w4")
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()
tiles = args.tiles.split(",")
dev = torch.device("cuda:0")
lib = _lib.load()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


M = 223839
SHAPES = [(1024, K) for K in (128, 192, 256, 320, 384, 480, 512)] + [(768, 256)]
say(f"M = {M}, residual + stat_partial, f32h, {args.launches} launches per row; us = in-situ profiler time of the contraction class per launch")
say(f"{'tile':10s} {'class':24s} {'N':>5s} {'K':>4s} {'us':>8s} {'TFLOP/s':>8s} {'TB/s':>6s} {'loop us':>8s}  C vs {tiles[0]:10s} max |d mean|, max rel d rstd")
for N, K in SHAPES:
    torch.manual_seed(K + N)
    A = torch.randn(M, K, device=dev)
    W = torch.randn(N, K, device=dev) * 0.05
    R = torch.randn(M, N, device=dev)
    W2h, cs = ops.split_weights_h2(W)
    am = ops.amax(A)
    out = torch.empty(M, N, device=dev)
    part = torch.empty(M, 2 * ((N + 63) // 64), 2, device=dev)
    stats = torch.empty(M, 2, device=dev)
    kw = dict(C_out=out, R=R, precision=3, W2h=W2h, col_scale=cs, a_amax=am, want_row_stats=True, stat_bufs=(part, stats))
    ref_c = ref_s = None
    for tile in tiles:
        lib.dzn_op_set_gemm_cfg(tile.encode())
        try:
            out.fill_(float("nan"))
            for _ in range(3):
                ops.gemm(A, W, **kw)
            torch.cuda.synchronize()
            _lib.profile_enable(True)
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(args.launches):
                ops.gemm(A, W, **kw)
            en.record()
            torch.cuda.synchronize()
            prof = [p for p in _lib.profile_collect() if p["name"].startswith("gemm_")]
        finally:
            _lib.profile_enable(False)
            lib.dzn_op_set_gemm_cfg(b"auto")
        assert len(prof) == 1 and prof[0]["launches"] == args.launches, prof
        dt = prof[0]["ms"] / prof[0]["launches"] * 1e-3
        loop = st.elapsed_time(en) / args.launches * 1e3
        alg_bytes = 4.0 * (M * K + 2 * M * N) + 4.0 * N * K
        if ref_c is None:
            ref_c, ref_s = out.clone(), stats.clone()
            same, ds = "reference", (0.0, 0.0)
        else:
            same = "bit-identical" if torch.equal(ref_c, out) else f"DIFFERENT ({int((ref_c != out).sum())} elements)"
            ds = (float((stats[:, 0] - ref_s[:, 0]).abs().max()), float(((stats[:, 1] - ref_s[:, 1]).abs() / ref_s[:, 1]).max()))
        say(f"{tile:10s} {prof[0]['name']:24s} {N:5d} {K:4d} {dt * 1e6:8.1f} {2.0 * M * N * K / dt / 1e12:8.1f} {alg_bytes / dt / 1e12:6.2f} "
            f"{loop:8.1f}  {same:18s} {ds[0]:.2e} {ds[1]:.2e}")
    del ref_c, ref_s
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
