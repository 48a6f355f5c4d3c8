"""Resegmentation on the MI355X: dzn_match_counts (csrc/reseg.hip) against its numpy twin at the tile edges and at the 4 h
size, the device composition (postprocess.resegment_device) against the reference's own run (tests/golden/
resegmentation_ref.npz, scripts/gen_resegmentation_golden.py) bit for bit, and the public pipeline (diarizen_amd/
resegmentation.py) end to end."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from _reseg_cases import CASES, GOLD, case_inputs, check_against_golden, renamed_runs_agree

WAV = os.path.join(GOLD, "EN2002a_30s.wav")
HYPOTHESIS = os.path.join(GOLD, "e2e_EN2002a_30s.rttm")

pytestmark = pytest.mark.gpu


def _operands(Cn, L, S, K, l0, seed=0):
    """decisions, a hypothesis matrix and first rows whose last window runs past Tr"""
    g = np.random.default_rng(seed + 7 * Cn + L)
    Lt = L - 2 * l0
    seg = (g.random((Cn, L, S)) < 0.4).astype(np.uint8)
    Tr = 11 * (Cn - 1) + max(Lt, 1) - (1 + max(Lt, 1) // 3)          # the last window's rows: Tr - its first row < Lt
    ref = (g.random((Tr, K)) < 0.5).astype(np.uint8)
    rows = (11 * np.arange(Cn)).astype(np.int32)
    return seg, ref, rows, Lt


@pytest.mark.parametrize("l0", [0, 3])
@pytest.mark.parametrize("Cn,L,S,K", [(3, 7, 4, 1), (3, 64, 4, 4), (2, 65, 4, 5), (1, 1, 4, 0), (5, 399, 4, 32), (4, 799, 3, 2)])
def test_match_counts_equal_numpy_twin(built_lib, gpu, Cn, L, S, K, l0):
    """L' not a multiple of 64, L' = 1, K = 0, n = 32, one word and several, rows past Tr: every count exactly.  A trim that
    leaves no frame (L = 1, l0 = 3) is DZN_E_INVALID."""
    import torch
    from diarizen_amd._lib import DznError
    from diarizen_amd.postprocess import match_counts_device, match_counts_host
    seg, ref, rows, Lt = _operands(Cn, L, S, K, l0)
    seg_t = torch.from_numpy(seg).to(gpu)
    if Lt < 1:
        with pytest.raises(DznError, match="invalid"):
            match_counts_device(seg_t, ref, rows, l0, Lt, K)
        return
    assert rows[-1] + Lt > len(ref)
    got = match_counts_device(seg_t, ref, rows, l0, Lt, K)
    want = match_counts_host(seg, ref, rows, l0, Lt, K)
    assert got.dtype == np.int32 and got.shape == (Cn, max(K, S), max(K, S))
    assert np.array_equal(got, want)
    assert want.any() or L == 1
    collect = getattr(built_lib, "dzn_checked_collect_reseg", None)        # a checked build (csrc/checked.h) carries index assertions
    if collect is not None:
        words = (C.c_uint * 4)()
        assert collect(words, 0) == 0 and words[0] == 0, [hex(w) for w in words]


def test_abi_rejects_bad_arguments_and_zero_windows_is_a_noop(built_lib, gpu):
    import torch
    lib = built_lib
    seg = torch.zeros((2, 10, 4), dtype=torch.uint8, device=gpu)
    ref = torch.ones((12, 33), dtype=torch.uint8, device=gpu)
    row = torch.zeros(2, dtype=torch.int32, device=gpu)
    out = torch.full((2 * 32 * 32,), -7, dtype=torch.int32, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(Cn=2, L=10, S=4, Tr=12, K=4, l0=0, Lt=10, seg_=True, row_=True, out_=True):
        return lib.dzn_match_counts(p(seg) if seg_ else None, p(ref), Cn, L, S, Tr, K, p(row) if row_ else None, l0, Lt,
                                    p(out) if out_ else None, st)
    for kw in (dict(K=33), dict(S=33, K=0), dict(S=0), dict(Lt=0), dict(l0=1), dict(l0=-1, Lt=5), dict(l0=8, Lt=3), dict(Cn=-1),
               dict(K=-1), dict(Tr=-1), dict(L=0), dict(seg_=False), dict(row_=False), dict(out_=False)):
        assert call(**kw) == -1, kw
    assert call(Cn=0) == 0 and call(Cn=0, seg_=False, row_=False, out_=False) == 0
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0                                          # nothing was launched so far
    assert call(K=32) == 0
    torch.cuda.synchronize()
    assert int(out.min()) >= 0


def test_four_hour_counts_equal_matmul_form(built_lib, gpu):
    """17 991 windows of 399 frames, K = 8 > S = 4: |a - b| summed = sum a + sum b - 2 a.b on {0,1} data, as float32 matrix
    products in numpy (exact: every sum is below 2^24)"""
    import torch
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import match_counts_device, receptive_field, reference_rows
    Cn, L, S, K = 17991, 399, 4, 8
    g = np.random.default_rng(11)
    tog = g.random((Cn, L, S)) < 0.03
    tog[:, 0, :] = g.random((Cn, S)) < 0.4
    seg = (np.cumsum(tog, axis=1) % 2).astype(np.uint8)
    rows = reference_rows(Cn, SlidingWindow(start=0.0, duration=8.0, step=0.8), receptive_field())
    Tr = int(rows[-1]) + L - 25                                                 # the last window runs past Tr
    rtog = g.random((Tr, K)) < 0.01
    ref = (np.cumsum(rtog, axis=0) % 2).astype(np.uint8)
    got = match_counts_device(torch.from_numpy(seg).to(gpu), ref, rows, 0, L, K)
    refpad = np.zeros((int(rows[-1]) + L, K), dtype=np.float32)
    refpad[:Tr] = ref
    for c0 in range(0, Cn, 3000):
        c1 = min(c0 + 3000, Cn)
        a = refpad[rows[c0:c1, None] + np.arange(L)[None, :]]                   # [c, L, K]
        b = np.zeros((c1 - c0, L, K), dtype=np.float32)
        b[:, :, :S] = seg[c0:c1]
        want = a.sum(axis=1)[:, :, None] + b.sum(axis=1)[:, None, :] - 2.0 * np.matmul(a.transpose(0, 2, 1), b)
        assert np.array_equal(got[c0:c1], want.astype(np.int32)), c0


@pytest.mark.parametrize("name", CASES)
def test_device_composition_equals_reference_run(built_lib, gpu, name):
    """decisions on the device -> dzn_match_counts -> assignment -> dzn_speaker_count / dzn_cluster_activations (warm_up 0) or
    the numpy aggregation (warm_up 0.05) -> RTTM: the counts, the discrete diarization and the RTTM bytes of the reference"""
    import torch
    from diarizen_amd.postprocess import receptive_field, resegment_device
    from _reseg_cases import G
    seg, _, chunks, w, _ = case_inputs(name)
    steps = []
    out = resegment_device(torch.from_numpy(np.ascontiguousarray(seg)).to(gpu), G[f"{name}_ref"], chunks, receptive_field(), w,
                           lambda step, artifact: steps.append(step))
    assert steps == ["speaker_counting", "permutated"]
    check_against_golden(name, seg, chunks, w, *out)


def test_more_than_32_speakers_take_the_numpy_path(built_lib, gpu):
    import torch
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import receptive_field, resegment_device, resegment_host
    seg, ref, _, _ = _operands(3, 99, 4, 33, 0)
    chunks = SlidingWindow(start=0.0, duration=2.0, step=0.2)
    got = resegment_device(torch.from_numpy(seg).to(gpu), ref, chunks, receptive_field())
    want = resegment_host(seg, ref, chunks, receptive_field())
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3].data, want[3].data) and got[3].data.shape[1] == 33


@pytest.fixture(scope="module")
def diar_pipeline(built_lib, gpu):
    """the seeded turn-taking weights of tests/test_detection_gpu.py"""
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    pipe = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield pipe
    pipe.close()


def _host_expectation(decisions, hypothesis, uri, num_samples, chunks, warm_up=0.0):
    from diarizen_amd.postprocess import discretize_turns, receptive_field, reference_extent, resegment_host
    from diarizen_amd.resegmentation import annotation_from_discrete
    frames = receptive_field()
    _, Tr = reference_extent(num_samples, 16000, chunks, frames)
    ref, labels = discretize_turns(hypothesis, frames, Tr)
    count, counts, hard, discrete = resegment_host(decisions, ref, chunks, frames, warm_up)
    return ref, labels, count, hard, discrete, annotation_from_discrete(discrete, uri=uri).to_rttm()


def test_pipeline_end_to_end_on_a_borrowed_engine(built_lib, gpu, tmp_path, diar_pipeline):
    """EN2002a_30s.wav, the hypothesis an RTTM file: the result, every hook artefact and the RTTM file are the host composition
    over the decisions the hook hands out; a second call gives the same bits; warm_up = 0.05 likewise; close() leaves the
    pipeline's engine open; DiariZenPipeline.resegment is the same call"""
    import wave as wavefile
    from diarizen_amd.core import Annotation
    from diarizen_amd.postprocess import permutated_decisions, trim_frames
    from diarizen_amd.resegmentation import Resegmentation, as_hypothesis
    with wavefile.open(WAV) as f:
        num_samples = f.getnframes()
    file = {"audio": WAV, "uri": "EN2002a"}
    hyp = as_hypothesis(HYPOTHESIS, "EN2002a")
    assert len({t[2] for t in hyp}) >= 2
    reseg = Resegmentation(diar_pipeline, rttm_out_dir=str(tmp_path))
    assert reseg.engine is diar_pipeline.engine and reseg.parameters() == reseg.default_parameters()
    calls = []

    def hook(step, artifact, file=None, completed=None, total=None):
        calls.append((step, artifact, file))
    ann = reseg(file, diarization=HYPOTHESIS, hook=hook)
    assert isinstance(ann, Annotation) and ann.uri == "EN2002a" and all(c[2] is file for c in calls)
    arte = [(s, a) for s, a, _ in calls if a is not None]
    assert [s for s, _ in arte] == ["segmentation", "speaker_counting", "@resegmentation/original",
                                    "@resegmentation/permutated", "discrete_diarization"]
    arte = dict(arte)
    decisions = np.asarray(arte["segmentation"].data)
    assert decisions.dtype == np.uint8 and decisions.shape == (29, 399, 4)
    ref, labels, count, hard, discrete, rttm = _host_expectation(decisions, hyp, "EN2002a", num_samples, reseg.chunks_window())
    assert reseg.labels == labels and len(labels) >= 2
    assert np.array_equal(arte["@resegmentation/original"].data, ref)
    assert np.array_equal(arte["speaker_counting"].data, count.data)
    n = max(len(labels), 4)
    assert arte["@resegmentation/permutated"].shape == (29, 4)
    assert np.array_equal(permutated_decisions(decisions, arte["@resegmentation/permutated"], n),
                          permutated_decisions(decisions, hard, n))
    assert np.array_equal(arte["discrete_diarization"].data, discrete.data)
    assert ann.to_rttm() == rttm and len(rttm.splitlines()) > 10
    assert (tmp_path / "EN2002a.rttm").read_text() == rttm
    assert reseg(file, diarization=hyp).to_rttm() == rttm                       # again, the hypothesis as turns, no hook
    assert reseg({**file, "diarization": open(HYPOTHESIS).read()}).to_rttm() == rttm     # RTTM text under the file's key
    # warm_up: the trimmed windows, matched on the device, aggregated by numpy
    reseg.instantiate({"warm_up": 0.05, "min_duration_on": 0.2})
    l0, Lt = trim_frames(399, 0.05)
    got = reseg(file, diarization=hyp)
    want = _host_expectation(decisions, hyp, "EN2002a", num_samples, reseg.chunks_window(), 0.05)[4]
    shell = Resegmentation.__new__(Resegmentation)
    shell.min_duration_on, shell.min_duration_off = 0.2, 0.0
    want_ann = shell._regions(want.data, want.sliding_window, "EN2002a", None)
    assert got.to_rttm() == want_ann.to_rttm() and got.to_rttm() != rttm and (l0, Lt) == (20, 359)
    reseg.instantiate(reseg.default_parameters())
    # an empty hypothesis: four speakers nobody named
    empty = reseg(file, diarization="")
    assert reseg.labels == [] and empty.to_rttm() == _host_expectation(decisions, [], "EN2002a", num_samples,
                                                                        reseg.chunks_window())[5]
    reseg.close()
    # the borrowed engine is still open: the pipeline's shortcut runs on it and gives the same bits
    again, names = diar_pipeline.resegment(file, HYPOTHESIS)
    assert again.to_rttm() == rttm and names == labels
    assert diar_pipeline.engine is reseg.engine


def test_renamed_hypothesis_moves_the_label_map(built_lib, gpu, diar_pipeline):
    """the same turns under names that sort differently: `labels` is the new sorted list, the result is the host composition
    of the renamed hypothesis, and it is the old result with its columns moved wherever to_diarization has no tie to break by
    column order (tests/_reseg_cases.py: boundary_ties)"""
    import torch
    import wave as wavefile
    from diarizen_amd.postprocess import receptive_field, resegment_device
    from diarizen_amd.resegmentation import Resegmentation, as_hypothesis
    with wavefile.open(WAV) as f:
        num_samples = f.getnframes()
    file = {"audio": WAV, "uri": "EN2002a"}
    hyp = as_hypothesis(HYPOTHESIS, "EN2002a")
    old = sorted({t[2] for t in hyp}, key=str)
    rename = {x: f"name{len(old) - 1 - k}" for k, x in enumerate(old)}          # the sorted order reversed
    reseg = Resegmentation(diar_pipeline)
    got = {}
    ann = reseg(file, diarization=[(a, b, rename[x]) for a, b, x in hyp], hook=lambda s, a, **kw: got.update({s: a}))
    assert reseg.labels == sorted(rename.values()) == [rename[x] for x in reversed(old)]
    decisions = np.asarray(got["segmentation"].data)
    want = _host_expectation(decisions, [(a, b, rename[x]) for a, b, x in hyp], "EN2002a", num_samples, reseg.chunks_window())
    assert ann.to_rttm() == want[5]
    seg_t = torch.from_numpy(decisions).to(gpu)
    renamed_runs_agree(decisions, hyp, rename, reseg.chunks_window(), num_samples,
                       lambda ref: resegment_device(seg_t, ref, reseg.chunks_window(), receptive_field()))


def test_from_a_hub_directory(built_lib, gpu, tmp_path, diar_pipeline):
    """a hub directory gives a segmentation-only engine of its own, closed by close(); same bits as on the borrowed engine"""
    import torch
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.resegmentation import Resegmentation
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import turn_taking_state_dict
    hub = tmp_path / "hub"
    hub.mkdir()
    (hub / "config.toml").write_text(
        '[model]\npath = "diarizen.models.eend.model_wavlm_conformer.Model"\n[model.args]\n'
        + "".join(f'{k} = {v!r}\n'.replace("'", '"') for k, v in E2E_CONFIG["model"]["args"].items())
        + "[inference.args]\nseg_duration = 8\nsegmentation_step = 0.1\nbatch_size = 32\napply_median_filtering = true\n")
    torch.save(turn_taking_state_dict(get_seg_config("wavlm_large_s80_md"), 0), hub / "pytorch_model.bin")
    file = {"audio": WAV, "uri": "EN2002a"}
    reseg = Resegmentation.from_pretrained(str(hub), device=gpu)
    assert reseg.engine.has_embedding == 0 and reseg.engine is not diar_pipeline.engine
    ann = reseg(file, diarization=HYPOTHESIS)
    reseg.close()
    assert reseg._owned is None
    assert ann.to_rttm() == diar_pipeline.resegment(file, HYPOTHESIS)[0].to_rttm()
