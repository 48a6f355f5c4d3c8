"""Per-speaker activity scores on the MI355X: dzn_speaker_scores (csrc/post.hip) against the reference's own clustered
aggregation (tests/golden/scores_ref.npz, scripts/gen_scores_golden.py) and the numpy restatement bit for bit; the classifier
kernel's soft multilabel output (dzn_segment_forward_soft) against its own log-probabilities and the reference-made soft
goldens; WindowRunner(with_scores=True); and DiariZenPipeline(return_scores=True) / get_segmentations end to end."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")
G = np.load(os.path.join(GOLD, "scores_ref.npz"))
AGG = [str(c) for c in G["agg_cases"]]

pytestmark = pytest.mark.gpu


def case(name):
    from diarizen_amd.core import SlidingWindow
    dur, ratio, n, w0, w1 = (float(v) for v in G[f"{name}_args"])
    return (G[f"{name}_soft"], G[f"{name}_hard"], SlidingWindow(start=0.0, duration=dur, step=ratio * dur), (w0, w1),
            len(G[f"{name}_scores"]))


# ----------------------------------------------------------------------------- dzn_speaker_scores
@pytest.mark.parametrize("name", AGG)
def test_device_scores_equal_reference_run_and_host(built_lib, gpu, name):
    """every bit of the reference's aggregate (cropped and warm-up cases included) and of postprocess.speaker_scores"""
    import torch
    from diarizen_amd.postprocess import DevicePost, receptive_field, speaker_scores
    soft, hard, chunks, warm_up, T = case(name)
    Cn, L, S = soft.shape
    post = DevicePost(np.zeros((Cn, L, S), dtype=np.uint8), chunks, receptive_field(), gpu)
    got = post.speaker_scores(hard, torch.from_numpy(soft).to(gpu), num_frames=T, warm_up=warm_up)
    ref = G[f"{name}_scores"]
    assert got.data.dtype == np.float32 and got.data.shape == ref.shape
    assert got.sliding_window.start == 0.0 and got.sliding_window.step == 0.02
    bad = np.nonzero(got.data.view(np.uint32) != ref.view(np.uint32))
    print(f"[{name}] {ref.size} scores, {len(bad[0])} differ from the reference run")
    assert np.array_equal(got.data.view(np.uint32), ref.view(np.uint32)), (name, bad[0][:5], bad[1][:5])
    host = speaker_scores(soft, chunks, receptive_field(), hard, warm_up=warm_up).data
    full = post.speaker_scores(hard, torch.from_numpy(soft).to(gpu), warm_up=warm_up).data     # T = every frame
    assert np.array_equal(full.view(np.uint32), host.view(np.uint32))
    torch.cuda.synchronize()


def test_more_than_32_clusters_take_the_host_function(built_lib, gpu):
    import torch
    from diarizen_amd.postprocess import DevicePost, receptive_field, speaker_scores
    soft, _, chunks, _, _ = case("w2s_k32")
    Cn, L, S = soft.shape
    hard = (np.arange(Cn * S, dtype=np.int8).reshape(Cn, S))        # 40 clusters, one local speaker each
    post = DevicePost(np.zeros((Cn, L, S), dtype=np.uint8), chunks, receptive_field(), gpu)
    got = post.speaker_scores(hard, torch.from_numpy(soft).to(gpu)).data
    assert got.shape[1] == 40 and np.array_equal(got, speaker_scores(soft, chunks, receptive_field(), hard).data)
    none = post.speaker_scores(np.full_like(hard, -2), torch.from_numpy(soft).to(gpu), num_frames=17).data
    assert none.shape == (17, 0)


def test_abi_rejects_bad_arguments(built_lib, gpu):
    import torch
    lib = built_lib
    soft = torch.full((3, 10, 4), 0.25, dtype=torch.float32, device=gpu)
    hard = torch.tensor([[0, 1, -2, 1]] * 3, dtype=torch.int8, device=gpu)
    start = torch.tensor([0, 5, 10], dtype=torch.int32, device=gpu)
    w = torch.ones(10, dtype=torch.float64, device=gpu)
    sc = torch.full((20, 32), -1.0, dtype=torch.float32, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(soft_=True, hard_=True, start_=True, ham_=True, wu_=True, sc_=True, Cn=3, L=10, S=4, T=20, K=2):
        return lib.dzn_speaker_scores(p(soft) if soft_ else None, p(hard) if hard_ else None, Cn, L, S,
                                      p(start) if start_ else None, p(w) if ham_ else None, p(w) if wu_ else None, T, K,
                                      p(sc) if sc_ else None, st)
    assert call() == 0
    torch.cuda.synchronize()
    out = sc.cpu().numpy().reshape(-1)[:40].reshape(20, 2)
    assert np.array_equal(out, np.full((20, 2), 0.25, dtype=np.float32))          # unit weights: the average of equal scores
    assert float(sc.reshape(-1)[40:].max()) == -1.0                                  # nothing written past [T, K]
    for kw in (dict(K=0), dict(K=33), dict(S=9), dict(S=0), dict(soft_=False), dict(hard_=False), dict(start_=False),
               dict(ham_=False), dict(wu_=False), dict(sc_=False), dict(L=0), dict(T=0), dict(Cn=-1)):
        assert call(**kw) == -1, kw


# ----------------------------------------------------------------------------- classifier epilogue (dzn_segment_forward_soft)
STRICT = ("f32", "f32s", "f32h")


@pytest.mark.parametrize("precision", STRICT + ("f16",))
def test_segment_soft_output(built_lib, gpu, precision):
    """tiny_ln (the smallest seeded config of tests/test_seg_gpu.py), one and three windows.  On the same call's outputs:
    logp and the u8 decisions are the bytes of the call without want_soft; soft == exp(logp) @ mapping evaluated in float64
    from that call's device logp within 1e-6 (at most 7 terms in [0, 1], a few ulp of expf each, float32 summation).
    Against the reference (strict modes): within 1.01e-3 of the reference-made soft golden — the strict bar |dlogp| <= 1e-3
    on probabilities that sum to at most 1 (|d exp(x)| <= exp(x) * (e^1e-3 - 1), summed over the classes of a speaker);
    f16 has its own reduced bar for logp, which the soft output inherits: not asserted here."""
    import torch
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.engine import Engine
    from oracle import seg_model
    from oracle.gen_golden import synth_wave
    cfg = get_seg_config("tiny_ln")
    g = np.load(os.path.join(GOLD, "seg_tiny_ln.npz"))
    assert int(g["B"]) == 2
    wave2 = synth_wave(2, int(g["N"]), int(g["wave_seed"]))
    eng = Engine(cfg, seg_model.seg_state_dict(cfg, int(g["weight_seed"])), max_batch=3, max_samples=int(g["N"]),
                 precision=precision, device=gpu)
    mapping = G["mapping_4_2"].astype(np.float64)
    ref_soft = G["seg_tiny_ln_soft"]
    for rows in ([0], [0, 1, 0]):
        wave = wave2[rows].contiguous().to(gpu)
        logp0, ml0 = eng.segment(wave)
        logp, ml, soft = eng.segment(wave, want_soft=True)
        only = eng.segment(wave, want_logp=False, want_multilabel=False, want_soft=True)
        torch.cuda.synchronize()
        assert torch.equal(logp.view(torch.int32), logp0.view(torch.int32)) and torch.equal(ml, ml0)
        assert only[0] is None and only[1] is None and torch.equal(only[2].view(torch.int32), soft.view(torch.int32))
        assert soft.shape == ml.shape and soft.dtype == torch.float32
        exp64 = np.exp(logp.cpu().numpy().astype(np.float64)) @ mapping
        err = float(np.abs(soft.cpu().numpy().astype(np.float64) - exp64).max())
        dref = float(np.abs(soft.cpu().numpy() - ref_soft[rows]).max())
        print(f"[tiny_ln {precision} B={len(rows)}] max|soft - exp(logp) @ mapping| = {err:.2e}, vs reference golden {dref:.2e}")
        assert err <= 1e-6
        if precision in STRICT:
            assert dref <= 1.01e-3
    eng.close()


# ----------------------------------------------------------------------------- runner + pipeline
@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    p = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield p
    p.close()


def test_runner_scores_leave_other_outputs_alone_and_are_batch_invariant(built_lib, gpu, pipe):
    """three 8 s windows of the recording: segmentations / embeddings bytes with and without with_scores, scores at batch
    1 vs 3; the scores are the raw soft output (no median filter) of Engine.segment"""
    import torch
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.inference import WindowRunner
    x = torch.from_numpy(np.ascontiguousarray(first_channel_16k(WAV, 16000)[:128000 + 2 * 12800], dtype=np.float32)).to(gpu)
    res = {}
    for bs in (1, 3):
        r = WindowRunner(pipe.engine, 8.0, 0.1, batch_size=bs, median_size=11)
        plain, scored = r.run(x), r.run(x, with_scores=True)
        torch.cuda.synchronize()
        assert plain.scores is None and scored.scores.shape == (3, r.num_frames, 4) and scored.scores.dtype == torch.float32
        assert torch.equal(plain.segmentations, scored.segmentations)
        assert torch.equal(plain.embeddings.view(torch.int32), scored.embeddings.view(torch.int32))
        res[bs] = scored
    assert torch.equal(res[1].scores.view(torch.int32), res[3].scores.view(torch.int32))
    assert torch.equal(res[1].segmentations, res[3].segmentations)
    _, _, soft = pipe.engine.segment(WindowRunner(pipe.engine, 8.0, 0.1, 3).windows_view(x).contiguous(), want_soft=True)
    assert torch.equal(soft.view(torch.int32), res[3].scores.view(torch.int32))


def test_pipeline_return_scores_end_to_end(built_lib, gpu, pipe, tmp_path):
    """EN2002a_30s.wav with the seeded turn-taking weights of the pipeline tests"""
    from diarizen_amd.clustering import active_speakers
    from diarizen_amd.core import SlidingWindowFeature
    from diarizen_amd.inference import WindowRunner
    from diarizen_amd.postprocess import crop_end, receptive_field, speaker_scores
    import torch
    base = pipe(WAV, sess_name="EN2002a")
    seen = {}
    inner = pipe.clustering

    def spy(**kw):
        out = inner(**kw)
        seen["hard"], seen["seg"] = np.array(out[0], copy=True), kw["segmentations"]
        return out
    steps = []
    pipe.clustering = spy
    pipe.rttm_out_dir = str(tmp_path)
    try:
        ann, scores = pipe(WAV, sess_name="EN2002a", return_scores=True,
                           hook=lambda step, art, **kw: steps.append((step, art)))
    finally:
        pipe.clustering = inner
        pipe.rttm_out_dir = None
    assert ann.to_rttm() == base.to_rttm() and (tmp_path / "EN2002a.rttm").read_text() == base.to_rttm()
    assert steps[-1][0] == "speaker_scores" and steps[-1][1] is scores
    hard = seen["hard"]
    hard[~active_speakers(seen["seg"])] = -2
    K = int(hard.max()) + 1
    assert isinstance(scores, SlidingWindowFeature) and scores.data.dtype == np.float32
    n = 480000
    grid = scores.sliding_window
    assert grid.start == 0.0 and grid.step == 0.02 and grid.duration == 0.025
    T = crop_end(10 ** 9, grid, n / 16000)
    assert K >= 2 and scores.data.shape == (T, K)               # the last window is zero-padded: cropped at the audio's end
    assert np.isfinite(scores.data).all() and scores.data.min() >= 0.0 and scores.data.max() <= 1.0 + 1e-6
    assert {lab for _, _, lab in ann.itertracks(yield_label=True)} <= set(range(K))
    soft = pipe.get_segmentations(WAV, soft=True)
    assert soft.data.shape == (29, 399, 4) and soft.data.dtype == np.float32
    assert soft.sliding_window.duration == 8.0 and soft.sliding_window.step == 0.1 * 8.0
    host = speaker_scores(soft.data, pipe.chunks_window(), receptive_field(), hard).data[:T]
    assert np.array_equal(scores.data.view(np.uint32), host.view(np.uint32))
    # soft=False: the hard decisions BEFORE the median filter
    raw = pipe.get_segmentations({"audio": WAV}, soft=False)
    from diarizen_amd.audio import first_channel_16k
    x = torch.from_numpy(np.ascontiguousarray(first_channel_16k(WAV, 16000), dtype=np.float32)).to(gpu)
    r0 = WindowRunner(pipe.engine, 8.0, 0.1, batch_size=32, median_size=0, exclude_overlap=False)
    exp = r0.run(x, with_embeddings=False).segmentations.cpu().numpy()
    assert raw.data.shape == exp.shape and np.array_equal(raw.data, exp)
    assert not np.array_equal(exp, seen["seg"])                 # the filter changed something on this recording
    assert set(np.unique(raw.data)) <= {0.0, 1.0}
