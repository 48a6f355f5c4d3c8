"""CPU check of the bounds test_attention_matrix_gpu.py holds the attention kernels to (tests/_attn_cases.py): on the exact
inputs of the matrix an IDEAL kernel per form — the form's operand rounding emulated in float64 (testkit/mx_emulation.py), fp32
accumulation with one rounding per step in two orders (forward: one softmax over the row, P.V key by key; blocked: online softmax
over 64-key tiles, P.V by 16 keys), an fp32 softmax — stays at least a factor 4 inside every bound.  So a ratio above 1 on the
device is the kernel's, not the derivation's.  The factor and its meaning are test_gemm_bounds_host.py's: it is asked of the
share of a bound that descends from accumulation and operand splitting (bound_acc); the single roundings enter at face value:
|error| <= bound_acc / 4 + (bound - bound_acc).

The emulation runs every window of the cases with L <= 129 (the first two windows — a quiet and a loud one in D4, the all-zero and a normal one in D6a — and, of more than three, the last) and one
(window, head) of each L = 399 and L = 798 case.  Also here: the input conditions the classes claim, on the float64 reference
alone.
"""
import pytest
import torch

import _attn_cases as ac

ROOM = 4.0
ORDERS = ("forward", "blocked")


def _ideal_ratio(form, shape, L, cls):
    inp, ref = ac.make_inputs(shape, L, cls), ac.launch_ref(shape, L, cls)
    B, h, heads = inp["B"], inp["h"], inp["heads"]
    q, k, v = ac.split_qkv(inp["qkv"], B, L, h)
    e, ea = ac.bound_of(ref, form)
    want = ref["out"].view(B, L, h, 64).permute(0, 2, 1, 3)
    e, ea = (x.view(B, L, h, 64).permute(0, 2, 1, 3) for x in (e, ea))
    windows = range(B) if B <= 2 else (0, 1, B - 1) if B > 3 else (0, 1)
    hs = slice(0, h) if L <= 129 else slice(h - 1, h)
    if L > 129:
        windows = (B - 1,)
    worst = 0.0
    for b in windows:
        gate_h = table_h = None
        if heads is not None:
            gate_h = inp["gate"].view(B, L, -1)[b][:, heads].T[hs]
            table_h = inp["table"][heads][hs]
        for order in ORDERS:
            got = ac.ideal_window(form, q[b, hs], k[b, hs], v[b, hs], gate_h, table_h, inp["amax"][b], L, order)
            err = (got - want[b, hs]).abs()
            lim = ea[b, hs] / ROOM + (e[b, hs] - ea[b, hs])
            assert torch.isfinite(got).all()
            bad = err > lim
            assert not bad.any(), (form, shape, L, cls, b, order, float((err[bad] / lim[bad]).max()) if (lim[bad] > 0).all() else "inf")
            worst = max(worst, float((err / lim.clamp_min(1e-300))[err > 0].max()) if (err > 0).any() else 0.0)
    return worst


@pytest.mark.parametrize("cls", ac.CLASSES)
def test_ideal_kernel_keeps_a_factor_4_under_every_bound_on_the_matrix_inputs(cls):
    worst = {}
    for shape, L, c, strided in ac.cases():
        if c != cls or strided:           # strided: the same inputs as the contiguous case; strides do not enter the arithmetic
            continue
        for form in ac.FORMS:
            worst[form] = max(worst.get(form, 0.0), _ideal_ratio(form, shape, L, cls))
    print(f"[{cls}] worst ideal-kernel error / (bound_acc / 4 + bound_rounding) per form: "
          + ", ".join(f"{f} {r:.3f}" for f, r in worst.items()))
    assert len(worst) == len(ac.FORMS) and max(worst.values()) <= 1.0


@pytest.mark.parametrize("fault,shape,L,cls,forms", [
    ("leak", "S5", 65, "D6b", ac.FORMS), ("leak", "S2", 17, "D1", ac.FORMS), ("norescale", "S5", 129, "D2g", ac.FORMS),
    ("norescale", "S2", 129, "D1", ac.FORMS), ("single", "S5", 65, "D1", ("f32h_split", "planes")),
    ("single", "S2", 129, "D3", ("f32h_split", "planes"))])
def test_subtly_wrong_kernels_break_the_bound(fault, shape, L, cls, forms):
    """the net is tight enough to matter: an ideal kernel with ONE thing wrong — a masked key of the partial last tile counted
    into the row sum, the accumulator missing one online-softmax factor, the lo terms of the fp16 split dropped — exceeds the
    bound of some element (the full bound, without the factor 4) on inputs of the matrix"""
    inp, ref = ac.make_inputs(shape, L, cls), ac.launch_ref(shape, L, cls)
    B, h, heads = inp["B"], inp["h"], inp["heads"]
    q, k, v = ac.split_qkv(inp["qkv"], B, L, h)
    b = B - 1
    gate_h = table_h = None
    if heads is not None:
        gate_h, table_h = inp["gate"].view(B, L, -1)[b][:, heads].T, inp["table"][heads]
    for form in forms:
        e = ac.bound_of(ref, form)[0].view(B, L, h, 64).permute(0, 2, 1, 3)[b]
        want = ref["out"].view(B, L, h, 64).permute(0, 2, 1, 3)[b]
        got = ac.ideal_window(form, q[b], k[b], v[b], gate_h, table_h, inp["amax"][b], L, "blocked", fault=fault)
        over = ((got - want).abs() > e)
        assert over.any(), (fault, form, shape, L, cls)
        print(f"[{fault} {form} {shape} L={L} {cls}] {int(over.sum())} of {over.numel()} elements over their bound")


def _cases_of(*classes):
    return [(s, L, c) for s, L, c, strided in ac.cases() if c in classes and not strided]


@pytest.mark.parametrize("shape,L,cls", _cases_of("D2g", "D2s"))
def test_d2_is_peaked_and_moves_the_running_maximum_as_claimed(shape, L, cls):
    ref = ac.launch_ref(shape, L, cls)
    pmax = torch.stack([w["pmax"] for w in ref["windows"]])
    assert float((pmax >= 0.9).double().mean()) >= 0.5
    s_std = float(torch.cat([(w["tile_max"]).reshape(-1) for w in ref["windows"]]).std())
    assert s_std > 0
    for w in ref["windows"]:
        run = torch.cummax(w["tile_max"], -1).values
        moved = run[..., 1:] > run[..., :-1]                # the running maximum after tile t against tile t - 1
        if cls == "D2g":
            assert moved.all()                              # every tile, every query
        else:
            assert not moved.any()                          # only the first tile sets it


@pytest.mark.parametrize("shape,L,cls", _cases_of("D2g"))
def test_d2_scores_have_the_spread_the_class_claims(shape, L, cls):
    inp = ac.make_inputs(shape, L, cls)
    q, k, _ = ac.split_qkv(inp["qkv"], inp["B"], L, inp["h"])
    s = ac.SCALE * q.double() @ k.double().transpose(-1, -2)
    assert 7.0 < float(s.std()) < 9.0


@pytest.mark.parametrize("shape,L,cls", _cases_of("D4"))
def test_d4_quiet_windows_are_2_to_the_10_below_their_loud_neighbours(shape, L, cls):
    inp, ref = ac.make_inputs(shape, L, cls), ac.launch_ref(shape, L, cls)
    B = inp["B"]
    o = ref["out"].view(B, -1).abs().amax(1)
    quiet, loud = o[0::2], o[1::2]
    assert L % 64 != 0 and loud.numel() and float(quiet.max()) < 2.0 ** -10 * float(loud.min())
    assert torch.equal(inp["amax"], inp["qkv"].view(B, -1).abs().amax(1))
    # the quiet windows are held to bounds of their own size: nothing of the neighbour's magnitude fits under them
    for f in ("f32", "f32h_split", "planes"):
        assert float(ref["bound"][f].view(B, -1)[0::2].max()) < 2.0 ** -10 * float(loud.min())


@pytest.mark.parametrize("shape,L,cls", _cases_of("D5"))
def test_d5_the_bias_decides_the_argmax(shape, L, cls):
    ref = ac.launch_ref(shape, L, cls)
    differ = torch.stack([(w["arg_s"] != w["arg_qk"]) for w in ref["windows"]])
    assert float(differ.double().mean()) >= 0.5


@pytest.mark.parametrize("shape,L,cls", _cases_of("D6a", "D6b"))
def test_d6_degenerate_inputs_are_what_they_claim(shape, L, cls):
    inp, ref = ac.make_inputs(shape, L, cls), ac.launch_ref(shape, L, cls)
    B, h = inp["B"], inp["h"]
    if cls == "D6a":
        assert float(inp["amax"][0]) == 0.0 and float(inp["amax"][1:].min()) > 0
        for f in ("f32", "f32h_split", "planes"):            # the bound of the zero window is exactly 0: only 0.0 passes
            assert float(ref["bound"][f].view(B, -1)[0].max()) == 0.0
        assert float(ref["out"].view(B, -1)[0].abs().max()) == 0.0
    else:
        v = inp["qkv"].view(B, L, -1)[:, :, 2 * h * 64:]
        assert torch.equal(v, v[:, :1].expand_as(v))
        assert float((ref["out"].view(B, L, -1) - v.double()).abs().max()) < 1e-14 * float(v.abs().max())


def test_case_table_covers_what_the_matrix_claims():
    cs = ac.cases()
    for s in ("S2", "S5"):
        assert {L for sh, L, c, st in cs if sh == s and c == "D1" and not st} == set(ac.LENGTHS)
    for s in ("S1", "S3", "S4", "S5b"):
        assert {L for sh, L, c, st in cs if sh == s and c == "D1"} == set(ac.SUB_LENGTHS)
    assert ("S6", 65, "D1", False) in cs and {L for sh, L, c, st in cs if st} == {65, 399}
    assert all(L >= 129 for sh, L, c, st in cs if c.startswith("D2")) and all(L % 64 for sh, L, c, st in cs if c == "D4")
    assert all(ac.has_bias(sh) for sh, L, c, st in cs if c == "D5")
    for shape, strided in (("S2", True), ("S5", False)):
        ldqkv, ldo = ac.strides(shape, strided)
        assert ldqkv % 4 == 0 and ldo >= ac.SHAPES[shape]["h"] * 64
    assert ac.strides("S2", True) == (3 * 5 * 64 + 8, 5 * 64 + 5)
