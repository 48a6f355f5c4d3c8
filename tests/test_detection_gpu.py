"""Voice activity / overlapped speech detection on the MI355X: dzn_detect (csrc/post.hip) against the reference's own
aggregation and binarisation (tests/golden/detection_ref.npz, scripts/gen_detection_golden.py) bit for bit, a 4 h-size
decision array against the host composition, and the public pipelines (diarizen_amd/detection.py) end to end."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")
G = np.load(os.path.join(GOLD, "detection_ref.npz"))
CASES = [str(c) for c in G["cases"]]
TASKS = {"speech": 1, "overlap": 2}

pytestmark = pytest.mark.gpu


def case_seg(name):
    src = str(G[f"{name}_src"])
    if src == "here":
        return G[f"{name}_seg"]
    f, key = src.split(":")
    return np.load(os.path.join(GOLD, f))[key]


def _chunks(name):
    from diarizen_amd.core import SlidingWindow
    dur, ratio, _ = G[f"{name}_args"]
    return SlidingWindow(start=0.0, duration=float(dur), step=float(ratio) * float(dur))


@pytest.mark.parametrize("name", CASES)
def test_device_scores_and_activity_equal_reference_run(built_lib, gpu, name):
    """both tasks in one launch (columns in bit order) and each alone: every score bit and every activity byte"""
    import torch
    from diarizen_amd.postprocess import detect_device, receptive_field
    seg = torch.from_numpy(np.ascontiguousarray(case_seg(name))).to(gpu)
    T = len(G[f"{name}_speech_scores"])
    act, sc, grid = detect_device(seg, _chunks(name), receptive_field(), 3, num_frames=T, want_scores=True)
    assert grid.start == 0.0 and grid.step == 0.02 and grid.duration == 0.025
    for k, task in enumerate(TASKS):
        ref = G[f"{name}_{task}_scores"][:, 0]
        assert np.array_equal(sc[:, k].view(np.uint32), ref.view(np.uint32)), (name, task)
        assert np.array_equal(act[:, k], G[f"{name}_{task}_active"]), (name, task)
        a1, s1, _ = detect_device(seg, _chunks(name), receptive_field(), TASKS[task], num_frames=T, want_scores=True)
        assert np.array_equal(s1[:, 0].view(np.uint32), ref.view(np.uint32)) and np.array_equal(a1[:, 0], act[:, k])
    assert not np.any(act[:, 1].astype(bool) & ~act[:, 0].astype(bool))      # overlap frames are speech frames
    torch.cuda.synchronize()


def synth_4h(seed=7, C=17991, L=399, S=4):
    """4 h of 8 s windows at a 0.8 s step: per (window, speaker) runs that toggle with probability 3 % per frame"""
    g = np.random.default_rng(seed)
    tog = g.random((C, L, S)) < 0.03
    tog[:, 0, :] = g.random((C, S)) < 0.4
    return (np.cumsum(tog, axis=1) % 2).astype(np.uint8)


@pytest.mark.parametrize("onset,offset", [(0.5, 0.5), (0.6, 0.4), (0.7, 0.55)])
def test_four_hour_decisions_equal_host_composition(built_lib, gpu, onset, offset):
    """17 991 windows (~720 k frames, more than one chunk per scan thread): device scores == numpy aggregate bit for bit,
    device hysteresis == the reference's frame loop (postprocess._hysteresis with Python-float thresholds, i.e. numpy's
    float32 comparison) for onset == offset and onset > offset"""
    import torch
    from diarizen_amd.core import SlidingWindow
    from diarizen_amd.postprocess import _hysteresis, detect_device, detection_scores_host, receptive_field
    seg = synth_4h()
    chunks = SlidingWindow(start=0.0, duration=8.0, step=0.1 * 8.0)
    segd = torch.from_numpy(seg).to(gpu)
    act, sc, _ = detect_device(segd, chunks, receptive_field(), 3, onset=onset, offset=offset, want_scores=True)
    assert len(sc) > 700_000
    for k, bit in enumerate((1, 2)):
        host = detection_scores_host(seg, chunks, receptive_field(), bit).data[:, 0]
        assert np.array_equal(sc[:, k].view(np.uint32), host.view(np.uint32))
        assert np.array_equal(act[:, k].astype(bool), _hysteresis(host, onset, offset))
    assert not np.any(act[:, 1].astype(bool) & ~act[:, 0].astype(bool))


def _hub(tmp_path, batch_size):
    import torch
    from diarizen_amd.configs import get_seg_config
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import turn_taking_state_dict
    hub = tmp_path / f"hub{batch_size}"
    hub.mkdir()
    a = E2E_CONFIG["model"]["args"]
    (hub / "config.toml").write_text(
        '[model]\npath = "diarizen.models.eend.model_wavlm_conformer.Model"\n[model.args]\n'
        + "".join(f'{k} = {v!r}\n'.replace("'", '"') for k, v in a.items())
        + f"[inference.args]\nseg_duration = 8\nsegmentation_step = 0.1\nbatch_size = {batch_size}\n"
          "apply_median_filtering = true\n")
    torch.save(turn_taking_state_dict(get_seg_config("wavlm_large_s80_md"), 0), hub / "pytorch_model.bin")
    return hub


def _gold_rttm(task):
    return G[f"EN2002a_{task}_rttm"].tobytes().decode()


@pytest.fixture(scope="module")
def diar_pipeline(built_lib, gpu):
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


def test_end_to_end_from_hub_directory_and_from_diarization_pipeline(built_lib, gpu, tmp_path, diar_pipeline):
    """EN2002a_30s.wav with the seeded turn-taking weights: the golden VAD / OSD RTTM (reference aggregate + Binarize on the
    raw decisions of the oracle forward), from a hub directory (segmentation-only engine) and from a DiariZenPipeline (its
    engine object, no second copy), at 64 and 1 windows per launch; RTTM files land in rttm_out_dir as <uri>.rttm"""
    from diarizen_amd.detection import OverlappedSpeechDetection, VoiceActivityDetection
    hub = _hub(tmp_path, 64)
    out = tmp_path / "rttm"
    file = {"audio": WAV, "uri": "EN2002a"}
    for cls, task in ((VoiceActivityDetection, "speech"), (OverlappedSpeechDetection, "overlap")):
        det = cls.from_pretrained(str(hub), rttm_out_dir=str(out / task), device=gpu)
        assert det.engine.has_embedding == 0 and det.engine.max_batch == 64
        assert det(file).to_rttm() == _gold_rttm(task)
        assert (out / task / "EN2002a.rttm").read_text() == _gold_rttm(task)
        ann = det(WAV)                                    # uri = the path's stem
        assert ann.uri == "EN2002a_30s" and ann.to_rttm() == _gold_rttm(task).replace(" EN2002a ", " EN2002a_30s ")
        det.close()
        for bs in (64, 1):
            shared = cls(diar_pipeline, batch_size=bs)
            assert shared.engine is diar_pipeline.engine and shared.engine.has_embedding == 1
            assert shared._runner.batch_size == bs
            assert shared(file).to_rttm() == _gold_rttm(task)


def test_hook_protocol_and_duration_parameters(built_lib, gpu, diar_pipeline):
    """hook: ("segmentation", None, completed=0, total=C) first, progress up to completed == total, then ("segmentation",
    aggregated scores [T, 1]) — all with file=file (PA/pipelines/voice_activity_detection.py:188-214, PA/core/inference.py:
    307-340); the scores are the golden's.  instantiate(min_duration_on / off) applies Binarize's support / removal to the
    regions of the default parameters."""
    from diarizen_amd.core import Annotation
    from diarizen_amd.detection import OverlappedSpeechDetection, VoiceActivityDetection
    file = {"audio": WAV, "uri": "EN2002a"}
    for cls, task in ((VoiceActivityDetection, "speech"), (OverlappedSpeechDetection, "overlap")):
        calls = []
        det = cls(diar_pipeline, batch_size=8)

        def hook(step, artifact, file=None, completed=None, total=None):
            calls.append((step, artifact, file, completed, total))
        base = det(file, hook=hook)
        assert base.to_rttm() == _gold_rttm(task)
        assert all(c[0] == "segmentation" and c[2] is file for c in calls)
        prog = [c for c in calls if c[1] is None]
        assert prog[0][3:] == (0, 29) and prog[-1][3:] == (29, 29) and len(prog) == 1 + 4
        assert [c[3] for c in prog] == sorted(c[3] for c in prog)
        last = calls[-1]
        assert last[1] is not None and last is calls[len(prog)]
        ref = G[f"EN2002a_{task}_scores"]
        assert np.array_equal(np.asarray(last[1].data).view(np.uint32), ref.view(np.uint32))
        det.instantiate({"min_duration_on": 0.5, "min_duration_off": 0.3})
        ann = det(file)
        exp = base.support(collar=0.3)
        for seg, tr in list(exp.itertracks()):
            if seg.duration < 0.5:
                del exp[seg, tr]
        assert isinstance(ann, Annotation) and ann.to_rttm() == exp.to_rttm()
        assert len(list(ann.itertracks())) < len(list(base.itertracks()))
        det.instantiate(det.default_parameters())
        assert det(file).to_rttm() == _gold_rttm(task)


def test_abi_rejects_bad_arguments(built_lib, gpu):
    import torch
    lib = built_lib
    seg = torch.zeros((3, 10, 4), dtype=torch.uint8, device=gpu)
    start = torch.tensor([0, 5, 10], dtype=torch.int32, device=gpu)
    w = torch.ones(10, dtype=torch.float64, device=gpu)
    sc = torch.empty((20, 2), dtype=torch.float32, device=gpu)
    act = torch.empty((20, 2), dtype=torch.uint8, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(seg_=True, start_=True, w_=True, sc_=True, Cn=3, L=10, S=4, T=20, tasks=3, onset=0.5, offset=0.5):
        return lib.dzn_detect(p(seg) if seg_ else None, Cn, L, S, p(start) if start_ else None, p(w) if w_ else None, T,
                              tasks, onset, offset, p(sc) if sc_ else None, p(act), st)
    assert call() == 0
    torch.cuda.synchronize()
    assert float(sc.abs().max()) == 0.0 and int(act.max()) == 0
    for kw in (dict(seg_=False), dict(start_=False), dict(w_=False), dict(sc_=False), dict(L=0), dict(T=0), dict(Cn=-1),
               dict(tasks=0), dict(tasks=4), dict(tasks=7), dict(S=9), dict(S=0), dict(onset=0.4, offset=0.6),
               dict(onset=float("nan"))):
        assert call(**kw) == -1, kw
