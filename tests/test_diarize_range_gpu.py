"""dzn_diarize_range (csrc/post.hip) on the MI355X: count, activations and the top-count selection against the arrays the
reference's own functions made (tests/golden/host_ref.npz, all seven cases); the concatenation of range calls equals the
[0, T) call byte for byte wherever the cuts fall; rows below the frontier do not depend on later windows; K = 32; bad
arguments are refused before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "host_ref.npz")
CASES = ["w2s_c60", "w2s_c200", "w5s_c40_step50", "w8s_c1", "w8s_c7_cap1", "w2s_c30_pad", "w2s_c25_s3"]

_REF = {}


def case(gpu, name):
    """per fixture case, once: device operands, the window grid and the whole-range result (host arrays, read-only)"""
    if name not in _REF:
        import torch
        from diarizen_amd.core import SlidingWindow
        from diarizen_amd.postprocess import _frame_grid, receptive_field
        g = np.load(GOLD)
        assert list(g["cases"]) == CASES
        seg, hard, args = g[f"{name}_seg"], g[f"{name}_hard"].astype(np.int8), g[f"{name}_args"]
        chunks = SlidingWindow(start=0.0, duration=float(args[0]), step=float(args[1]) * float(args[0]))
        _, starts, T = _frame_grid(seg.shape[0], seg.shape[1], chunks, receptive_field())
        K, max_count = g[f"{name}_binary"].shape[1], int(args[2])
        d = dict(seg=torch.from_numpy(seg).to(gpu), hard=torch.from_numpy(hard).to(gpu), start=torch.from_numpy(starts).to(gpu),
                 starts=starts, T=T, K=K, max_count=max_count, chunks=chunks, C=seg.shape[0],
                 gold=(g[f"{name}_count"].reshape(-1), g[f"{name}_binary"], g[f"{name}_activations"]))
        d["whole"] = run(d, 0, T)
        _REF[name] = d
    return _REF[name]


def run(d, t0, t1, num_windows=None, K=None):
    """one range call -> (count [n], active [n, K], activations [n, K]) on the host, read-only"""
    from diarizen_amd.postprocess import diarize_range_launch
    cnt, active, act = diarize_range_launch(d["seg"], d["hard"], d["C"] if num_windows is None else num_windows, d["start"],
                                            t0, t1, d["K"] if K is None else K, d["max_count"], want_activations=True)
    out = tuple(x.cpu().numpy() for x in (cnt, active, act))
    for x in out:
        x.setflags(write=False)
    return out


def run_ranges(d, cuts):
    bounds = [0] + [int(c) for c in cuts] + [d["T"]]
    assert bounds == sorted(bounds)
    parts = [run(d, a, b) for a, b in zip(bounds[:-1], bounds[1:])]
    for (a, b), p in zip(zip(bounds[:-1], bounds[1:]), parts):
        assert p[0].shape == (b - a,) and p[1].shape == p[2].shape == (b - a, d["K"])
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def assert_same(got, ref):
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_count_activations_and_selection_against_the_reference_made_arrays(built_lib, gpu, name):
    d = case(gpu, name)
    cnt, active, act = d["whole"]
    g_count, g_binary, g_act = d["gold"]
    T, K = d["T"], d["K"]
    assert len(g_count) == T and g_binary.shape == g_act.shape == (T, K)
    assert cnt.dtype == np.uint8 and active.dtype == np.uint8 and act.dtype == np.int32
    assert np.array_equal(cnt, g_count)
    assert np.array_equal(act, g_act)                                   # the reference's float32 sums of 0 / 1 are exact
    # frames with a tie at the selection boundary (the c-th and (c+1)-th largest activation are equal, 0 < c < K): the
    # reference's pick is numpy's sort order there; everywhere else the selected set is unique
    srt = -np.sort(-act, axis=1)
    c = np.minimum(cnt.astype(np.int64), K)
    inner = (c > 0) & (c < K)
    tied = inner & (srt[np.arange(T), np.maximum(c, 1) - 1] == srt[np.arange(T), np.minimum(c, K - 1)])
    print(f"{name}: T = {T}, K = {K}, {int(tied.sum())} tied frames ({tied.mean():.1%}), "
          f"{int((active != g_binary).any(axis=1).sum())} frames differ from the reference-made binary")
    assert tied.mean() <= 0.45
    assert np.array_equal(active[~tied], g_binary[~tied])
    # the kernel's own rule, on every frame: np.argsort(-act, kind="stable")
    order = np.argsort(-act, axis=1, kind="stable")
    want = np.zeros((T, K), np.uint8)
    np.put_along_axis(want, order, (np.arange(K)[None, :] < c[:, None]).astype(np.uint8), axis=1)
    assert np.array_equal(active, want)
    assert np.array_equal(active.sum(axis=1), c)


@pytest.mark.parametrize("name", ["w2s_c60", "w8s_c1", "w2s_c200", "w2s_c25_s3"])
def test_ranges_cut_at_window_starts_and_after_frame_zero(built_lib, gpu, name):
    d = case(gpu, name)
    T = d["T"]
    assert_same(run_ranges(d, [1]), d["whole"])                                        # [0, 1), then the rest
    assert_same(run_ranges(d, sorted(set(d["starts"][1:].tolist()))), d["whole"])      # a cut at every window start frame
    assert_same(run_ranges(d, [T // 2, T // 2, T - 1]), d["whole"])                    # an empty range, a last single frame


def test_rows_below_the_frontier_do_not_depend_on_later_windows(built_lib, gpu):
    from diarizen_amd.postprocess import committed_frames, receptive_field
    d = case(gpu, "w2s_c200")
    changed = 0
    for c in (1, 57, 199):
        F = committed_frames(c, d["chunks"], receptive_field())
        assert F == int(d["starts"][c]) and 0 < F < d["T"]
        end = int(d["starts"][c - 1]) + 99                                             # frames covered by windows 0 .. c - 1
        got = run(d, 0, end, num_windows=c)
        assert_same(tuple(x[:F] for x in got), tuple(x[:F] for x in d["whole"]))
        changed += int((got[2][F:] != d["whole"][2][F:end]).any())
    assert changed, "the provisional tail never differed from the final result: the case shows nothing"


def test_k_32_on_a_frame_count_off_the_block_grid(built_lib, gpu):
    """K = 32: one frame per 32 lanes, 8 frames per workgroup; T = 691 is no multiple of 256, 64 or 8.  Labels -2 and 32 (out
    of range) are skipped; max_count = 3 caps the count."""
    import torch
    from diarizen_amd.postprocess import diarize_range_host
    d = dict(case(gpu, "w2s_c60"))
    g = np.random.default_rng(7)
    hard = g.integers(-2, 33, size=(d["C"], 4)).astype(np.int8)
    hard[hard == -1] = 31
    assert {-2, 0, 31, 32} <= set(hard.reshape(-1).tolist())
    d.update(hard=torch.from_numpy(hard).to(gpu), K=32, max_count=3)
    assert d["T"] == 691
    got = run(d, 0, d["T"])
    seg = d["seg"].cpu().numpy()
    want = diarize_range_host(seg, hard, d["starts"], 0, d["T"], 32, 3)
    assert_same(got, want)
    assert int(got[0].max()) == 3 and int(case(gpu, "w2s_c60")["whole"][0].max()) == 4
    assert_same(run(d, 100, 333), tuple(x[100:333] for x in want))


def test_abi_rejects_bad_arguments_and_launches_nothing(built_lib, gpu):
    import torch
    lib = built_lib
    d = case(gpu, "w2s_c60")
    cnt = torch.full((40,), 9, dtype=torch.uint8, device=gpu)
    active = torch.full((40, 32), 9, dtype=torch.uint8, device=gpu)
    act = torch.full((40, 32), -7, dtype=torch.int32, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(t0, t1, K=4, S=4, max_count=20, cnt_=True, active_=True, act_=True):
        return lib.dzn_diarize_range(p(d["seg"]), p(d["hard"]), d["C"], 99, S, p(d["start"]), t0, t1, K, max_count,
                                     p(cnt) if cnt_ else None, p(active) if active_ else None, p(act) if act_ else None, st)
    for args, kw in (((-1, 5), {}), ((10, 9), {}), ((0, 10), dict(K=0)), ((0, 10), dict(K=33)), ((0, 10), dict(S=9)),
                     ((0, 10), dict(max_count=-1)), ((0, 10), dict(cnt_=False)), ((0, 10), dict(active_=False))):
        assert call(*args, **kw) == -1, (args, kw)
    assert call(12, 12) == 0 and call(0, 0, act_=False) == 0                        # empty: DZN_OK, no launch
    torch.cuda.synchronize()
    assert int(cnt.min()) == 9 == int(cnt.max()) and int(active.min()) == 9 == int(active.max())
    assert int(act.min()) == -7 == int(act.max())
    assert call(5, 15, act_=False) == 0                                             # the activations are optional
    torch.cuda.synchronize()
    whole = d["whole"]
    assert np.array_equal(cnt[:10].cpu().numpy(), whole[0][5:15]) and int(cnt[10:].min()) == 9
    flat = active.reshape(-1).cpu().numpy()
    assert np.array_equal(flat[:40].reshape(10, 4), whole[1][5:15]) and int(flat[40:].min()) == 9
    assert int(act.min()) == -7 == int(act.max())
