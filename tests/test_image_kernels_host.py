"""CPU: the bounds of tests/_image_cases.py are neither loose nor tight by accident.  For the convolution and the BasicBlock an IDEAL
fp32 kernel (operands split as the kernels split them, products added in fp32 one rounding per step, forward and in reverse) stays
inside the bound with a QUARTER of its accumulation share on every case of the tables, and each subtly wrong kernel of the lists
below falls outside the bound on at least one case.  The same references and bounds then judge the device kernels in
test_image_kernels_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _image_cases as ic
from _image_cases import F32, F64, worst_ratio

IDEAL_PIXELS = 700          # the ideal kernel runs on the first images of a launch's list up to about this many pixels: images are
                            # independent of each other in the arithmetic, and every image shape of the tables is reached


def _ideal_images(c):
    sel = ic.case_images(c)
    keep = max(1, min(len(sel), IDEAL_PIXELS // (c["H"] * c["W"])))
    zero = [b for b in sel if b == 2 and b not in sel[:keep] and c["H"] * c["W"] <= IDEAL_PIXELS]
    return sorted(sel[:keep] + zero)                                # ... and the empty image, where the list has it


def _ideal(cases):
    worst = 0.0
    for c in cases:
        if not ic.case_images(c):
            continue
        inp, imgs = ic.inputs(c), _ideal_images(c)
        run, bound = ic.RUN[c["kernel"]], ic.BOUND[c["kernel"]]
        ref, bnd = run(c, inp)["out"][imgs], bound(c, inp, 0.25)["out"][imgs]
        assert np.isfinite(bnd).all() and (bnd > 0).all(), f"an element of {c} has no bound"
        for order in ("forward", "reverse"):
            r = worst_ratio(run(c, inp, F32, order, images=imgs)["out"][imgs], ref, bnd)
            assert r <= 1.0, f"ideal fp32 kernel ({order} order) at {r:.3f} of the bound with a quarter of its accumulation share: {c}"
            worst = max(worst, r)
    print(f"ideal / (bound at s = 1/4): {worst:.3f}")


def _judge(c, inp, bound=None):
    """-> f(mutant) = worst error / bound of that wrong kernel over the images the launch lists"""
    sel = ic.case_images(c)
    run = ic.RUN[c["kernel"]]
    if not sel:
        return lambda mutant: 0.0
    ref = run(c, inp)["out"][sel]
    bnd = (ic.BOUND[c["kernel"]](c, inp) if bound is None else bound)["out"][sel]
    return lambda mutant: worst_ratio(run(c, inp, mutant=mutant)["out"][sel], ref, bnd)


def _mutants(cases, mutants):
    """-> {mutant: the first case that holds it outside the bound}"""
    caught, left = {}, list(mutants)
    for c in cases:
        if not left:
            break
        if c["B"] > 20 and left != ["stale_ring"]:       # the launches with more items than workgroups: what only they can show
            continue
        judge = _judge(c, ic.inputs(c))
        for m in list(left):
            if m == "lo_dropped" and c["np"] == 1:        # one term has no lo
                continue
            if judge(m) > 1.0:
                caught[m] = c
                left.remove(m)
    assert not left, f"no case of the table holds these wrong kernels outside the bound: {left}"
    for m, c in caught.items():
        print(f"{m}: outside the bound at {c}")
    return caught


def test_conv_ideal_kernel_is_inside_a_quarter_of_the_bound():
    _ideal(ic.conv_cases())


@pytest.mark.parametrize("C", [32, 64])
def test_block_ideal_kernel_is_inside_a_quarter_of_the_bound(C):
    _ideal(ic.block_cases(C))


def test_conv_wrong_kernels_are_outside_the_bound():
    caught = _mutants(ic.conv_cases(), ic.CONV_MUTANTS)
    assert caught["relu_after_residual_only"]["relu"] and caught["relu_after_residual_only"]["R"]
    assert caught["list_identity"]["zl"] == "subset"


@pytest.mark.parametrize("C", [32, 64])
def test_block_wrong_kernels_are_outside_the_bound(C):
    cases = ic.block_cases(C)
    caught = _mutants(cases, ic.BLOCK_MUTANTS)
    c = caught["stale_ring"]
    nitem, grid = ic.block_items(c)
    assert nitem > grid, f"stale_ring caught by a launch whose workgroups run one item each: {c}"
    assert caught["strip_seam"]["W"] > ic.STRIP


def test_stale_ring_is_invisible_without_a_second_item():
    """what the old tests could not see: below the slot count the wrong kernel IS the right one"""
    c = next(c for c in ic.block_cases(32) if c["zl"] == "none" and c["np"] == 2 and c["W"] > ic.STRIP and c["B"] < 20)
    inp = ic.inputs(c)
    assert np.array_equal(ic.block_run(c, inp, mutant="stale_ring")["out"], ic.block_run(c, inp)["out"])


@pytest.mark.parametrize("C", [32, 64])
def test_lo_dropped_fails_the_two_term_bound_and_passes_the_one_term_one(C):
    """the accumulation share (K + 8) u S is most of the two-term bound (2^-15.8 S at C = 32, 2^-14.8 S at C = 64), so a missing lo*hi
    product (about 2^-13 |w||x| per term, signs at random) is outside it on the cases named here, not on all; it is inside the
    one-term bound everywhere"""
    outside = []
    for c in ic.block_cases(C)[:24]:
        if c["np"] != 2 or not ic.case_images(c):
            continue
        inp = ic.inputs(c)
        one = _judge(c, inp, bound=ic.block_bound(dict(c, np=1), inp))("lo_dropped")
        assert one <= 1.0, f"a two-term kernel without its lo*hi product at {one:.3f} of the ONE-term bound: {c}"
        if _judge(c, inp)("lo_dropped") > 1.0:
            outside.append(c)
    assert outside, "no case holds a kernel without its lo*hi product outside the two-term bound"
    print(f"lo_dropped: outside the two-term bound at {outside}")


def test_mid_pad_leak_is_what_a_positive_b1_shows():
    """relu(b1) > 0 is what leaks when the intermediate outside the image is not forced to zero: with b1 <= 0 and a quiet image
    the same wrong kernel is far closer to the bound"""
    c = next(c for c in ic.block_cases(32) if c["np"] == 2 and c["zl"] == "none" and c["B"] >= 2 and c["H"] >= 2)
    inp = ic.inputs(c)
    assert (inp["b1"] > 0).any() and (inp["b1"] < 0).any() and np.abs(inp["b1"]).max() == 0.5
    quiet = [1]
    got, ref, bnd = (f(c, inp, **k)["out"][quiet] for f, k in ((ic.block_run, dict(mutant="mid_pad_live")), (ic.block_run, {}), (ic.block_bound, {})))
    assert worst_ratio(got, ref, bnd) > 1e3
    neg = dict(inp, b1=-np.abs(inp["b1"]))
    got, ref, bnd = (f(c, neg, **k)["out"][quiet] for f, k in ((ic.block_run, dict(mutant="mid_pad_live")), (ic.block_run, {}), (ic.block_bound, {})))
    assert worst_ratio(got, ref, bnd) < 1e3


def test_tables_reach_what_they_name():
    conv = ic.conv_cases()
    assert {(c["H"], c["W"]) for c in conv} == set(ic.CONV_SHAPES) and {c["B"] for c in conv} == set(ic.CONV_B)
    for nterm in (3, 2):
        mine = [c for c in conv if c["np"] == nterm]
        assert {(c["relu"], c["R"], c["post"]) for c in mine} == {(e["relu"], e["R"], e["post"]) for e in ic.EPILOGUES}
        assert {c["trk"] for c in mine} == set(ic.TRACKERS) and {c["zl"] for c in mine} == set(ic.LISTS)
        assert {c["amax8"] for c in mine} == {True, False}
        assert any(c["B"] == 17 for c in mine) and any(c["B"] > 8 and c["zl"] == "none" for c in mine)
        # more tiles per image than an XCD has workgroups, with more images than XCDs
        assert any(-(-c["H"] * (c["W"] + 2) // ic.CONV_TILE) > ic.CONV_GRID // 8 and c["B"] > 8 and c["zl"] == "none" for c in mine)
    for C in (32, 64):
        blk = ic.block_cases(C)
        assert {c["W"] for c in blk} == set(ic.BLOCK_W) and {c["H"] for c in blk} >= set(ic.BLOCK_H)
        for nterm in (2, 1):
            mine = [c for c in blk if c["np"] == nterm]
            assert {c["trk"] for c in mine} == set(ic.TRACKERS) and {c["zl"] for c in mine} == set(ic.LISTS)
            assert {c["l1x"] for c in mine} == {1.0, 8.0} and {c["amax8"] for c in mine} == {True, False}
            assert any(ic.block_items(c)[0] > ic.SLOTS[C] for c in mine)
            assert any(c["B"] >= 3 for c in mine)
    for c in conv + ic.block_cases(32) + ic.block_cases(64):
        assert c["B"] * (c["H"] + 2) * (c["W"] + 2) * c["C"] * 4 <= 12.5e6, c


def test_inputs_are_what_the_tables_promise():
    c = next(c for c in ic.conv_cases() if c["B"] >= 3 and not c["amax8"])
    inp = ic.inputs(c)
    assert not inp["x"][2].any() and inp["amax_in"][2] == 0                       # the empty image
    assert inp["amax_in"][0] / inp["amax_in"][1] > 2.0 ** 18                      # loud next to quiet
    assert np.array_equal(inp["amax_in"], np.abs(inp["x"]).reshape(c["B"], -1).max(1))
    for edge in (inp["x"][:, 0], inp["x"][:, -1], inp["x"][:, :, 0], inp["x"][:, :, -1]):
        assert not edge.any()
    c8 = next(c for c in ic.conv_cases() if c["amax8"])
    i8 = ic.inputs(c8)
    assert np.array_equal(i8["amax_in"], 8 * np.abs(i8["x"]).reshape(c8["B"], -1).max(1))
    w = ic.weights(32)
    assert w["l1max1"] >= np.abs(w["w1"]).astype(F64).sum(1).max()


def test_h2_scale_restates_split_h():
    a = np.asarray([1.0, 1.5, 2.0, 3e4, 65504.0, 2.0 ** -20, 7e-8, 1e30], F32)
    from testkit import mx_emulation as emu
    assert np.array_equal(ic.h2_scale(a), emu._pow2_scale_h2(torch.from_numpy(a)).numpy())
    assert (a.astype(F64) * ic.h2_scale(a) >= 2.0 ** 14).all() and (a.astype(F64) * ic.h2_scale(a) < 2.0 ** 15).all()
    # the fallbacks: an empty tracker, a negative one, a NaN, an infinity and an exponent above 100 give scale 1; below 2^-100 the clamp
    assert ic.h2_scale(np.asarray([0.0, -1.0, np.nan, np.inf, 2.0 ** 101], F32)).tolist() == [1.0] * 5
    assert ic.h2_scale(np.asarray([2.0 ** -120, 1e-45], F32)).tolist() == [2.0 ** 114] * 2
    assert ic.h2_scale(np.asarray([2.0 ** 100], F32)).tolist() == [2.0 ** -86]


def test_tracker_rules():
    """amax_out[b] = max(preload, max |out[b]|) bit for bit for the images of the list, untouched outside it and when absent —
    stated once in _image_cases.tracker_after, which the device test holds the kernels' trackers against"""
    seen = set()
    for c in ic.conv_cases() + ic.block_cases(32):
        if c["B"] > 20 or (c["trk"], c["zl"]) in seen:
            continue
        seen.add((c["trk"], c["zl"]))
        inp = ic.inputs(c)
        run = ic.RUN[c["kernel"]]
        ref = run(c, inp)["out"]
        pre = ic.tracker_preload(c, ref)
        sel = ic.case_images(c)
        out = ref.astype(F32)
        after = ic.tracker_after(c, pre, out)
        if c["trk"] == "absent":
            assert pre is None and after is None
            continue
        rest = [b for b in range(c["B"]) if b not in sel]
        assert np.array_equal(after[rest].view(np.uint32), pre[rest].view(np.uint32)) and (pre[rest] == 3.0).all()
        for b in sel:
            m = np.abs(out[b]).max()
            assert after[b].view(np.uint32) == max(pre[b], m).view(np.uint32)
            assert {"zero": pre[b] == 0 and after[b] == m, "above": pre[b] > m and after[b] == pre[b],
                    "below": (0 < pre[b] < m and after[b] == m) or m == 0}[c["trk"]], (c, b)
    assert seen >= {(t, z) for t in ic.TRACKERS for z in ("none", "subset")}


def test_reference_against_torch_conv2d():
    """the numpy reference against torch.nn.functional.conv2d in float64, once: guards the reference against a typo of its own"""
    F = torch.nn.functional
    nchw = lambda v: torch.from_numpy(np.ascontiguousarray(v, F64)).permute(0, 3, 1, 2)
    oihw = lambda w, C: torch.from_numpy(w.astype(F64)).reshape(C, 3, 3, C).permute(0, 3, 1, 2)
    conv = next(c for c in ic.conv_cases() if c["relu"] and c["R"] and c["zl"] == "none" and c["H"] > 1)
    inp = ic.inputs(conv)
    x = nchw(inp["x"][:, 1:-1, 1:-1])
    want = torch.relu(torch.relu(F.conv2d(x, oihw(inp["w1"], 32), torch.from_numpy(inp["b1"].astype(F64)), padding=1)) + nchw(inp["R"][:, 1:-1, 1:-1]))
    got = nchw(ic.conv_run(conv, inp)["out"])
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    for C in (32, 64):
        c = next(c for c in ic.block_cases(C) if c["zl"] == "none" and c["H"] > 2 and c["W"] > ic.STRIP and c["B"] > 1)
        inp = ic.inputs(c)
        x = nchw(inp["x"][:, 1:-1, 1:-1])
        b1, b2 = (torch.from_numpy(inp[k].astype(F64)) for k in ("b1", "b2"))
        mid = torch.relu(F.conv2d(x, oihw(inp["w1"], C), b1, padding=1))
        want = torch.relu(F.conv2d(mid, oihw(inp["w2"], C), b2, padding=1) + x)
        got = ic.block_run(c, inp)
        for b in range(c["B"]):       # per image: the loud ones would hide the quiet ones in one norm
            assert (nchw(got["out"])[b] - want[b]).abs().max() <= 1e-12 * max(want[b].abs().max(), 1e-30)
            assert (nchw(got["mid"])[b] - mid[b]).abs().max() <= 1e-12 * max(mid[b].abs().max(), 1e-30)
