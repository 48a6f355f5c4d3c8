"""BASELINE.json configs[0]: example/EN2002a_30s.wav through the drop-in DiariZenPipeline on the GPU
vs the oracle's execution of the reference device stage on CPU (tests/golden/e2e_EN2002a_30s.npz:
per-window hard decisions after the median filter + per-(window, speaker) embeddings) and the golden
RTTM tests/golden/e2e_EN2002a_30s.rttm, which was produced INDEPENDENTLY of the product's host stage: the
reference's own clustering module + oracle/host_stage.py (the reference's loops restated loop for loop).
Weights: the seeded TURN-TAKING weights (testkit/weights.py) — no hub weights exist offline, and plain
random weights emit one class for every frame; with these the fixture has 11 powerset classes (7 of them
>= 5 % of the frames), >= 8 transitions in every window, 31 % overlapped frames, both mask branches of
get_embeddings (89 clean / 25 fallback) and 3 speakers in the RTTM (asserted in tests/test_host.py).

Bars: decisions bit-exact (u8), embeddings cosine >= 0.9999, RTTM text identical to the golden file.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
WAV = os.path.join(GOLD, "EN2002a_30s.wav")


@pytest.fixture(scope="module", params=["f32", "f32s", "f32h"])
def pipeline(built_lib, gpu, request):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    from oracle.gen_golden import E2E_CONFIG
    import copy
    cfg = get_seg_config("wavlm_large_s80_md")
    return DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu,
                            precision=request.param, seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0))


def test_device_stage_matches_reference_execution(pipeline):
    from diarizen_amd.audio import first_channel_16k
    g = np.load(os.path.join(GOLD, "e2e_EN2002a_30s.npz"))
    wave = first_channel_16k(WAV)
    assert wave.shape == (480000,)
    seg, emb = pipeline.device_stage(wave)
    assert seg.shape == g["seg"].shape == (29, 399, 4)          # 30 s -> 29 windows of 8 s
    assert np.array_equal(seg, g["seg"])                         # bit-exact hard decisions
    e, r = torch.from_numpy(emb).reshape(-1, 256), torch.from_numpy(g["emb"]).reshape(-1, 256)
    cos = torch.nn.functional.cosine_similarity(e, r, dim=-1)
    assert cos.min().item() > 0.9999
    assert (e - r).abs().max().item() <= 1e-4 * r.abs().max().item()


def test_rttm_equal_and_api_surface(pipeline, tmp_path):
    g = np.load(os.path.join(GOLD, "e2e_EN2002a_30s.npz"))
    pipeline.rttm_out_dir = str(tmp_path)
    ann = pipeline(WAV, sess_name="EN2002a")
    assert ann.uri == "EN2002a"
    rttm = (tmp_path / "EN2002a.rttm").read_text()
    assert rttm == ann.to_rttm()
    ref = open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read()      # reference clustering + oracle/host_stage.py
    assert rttm == ref
    assert len({ln.split()[7] for ln in rttm.splitlines()}) >= 3
    for line in rttm.splitlines():
        f = line.split()
        assert f[0] == "SPEAKER" and f[1] == "EN2002a" and len(f) == 10
    t = pipeline.timings
    assert t["audio_s"] == 30.0 and t["device_s"] > 0
    # hook protocol of the pyannote pipeline (PA/pipelines/utils/hook.py:36-224; PA/core/inference.py:308-340)
    calls = []
    file = {"audio": WAV}
    ann2 = pipeline(file, sess_name="EN2002a",
                    hook=lambda name, artifact, file=None, total=None, completed=None:
                    calls.append((name, None if artifact is None else type(artifact).__name__, file, total, completed)))
    assert ann2.to_rttm() == rttm
    assert all(c[2] is file for c in calls)
    prog = [c for c in calls if c[0] == "segmentation" and c[1] is None]
    assert prog[0][3:] == (29, 0) and prog[-1][3:] == (29, 29)
    assert [c[0] for c in calls if c[1] is not None] == ["segmentation", "embeddings", "speaker_counting",
                                                         "discrete_diarization"]


def test_plugin_facades(pipeline, gpu):
    """[model].path facade: forward(waveforms[B,C,N]) -> logp[B,L,11]; embedding facade properties."""
    m = pipeline.segmentation_model
    x = torch.randn(2, 1, 128000) * 0.1
    logp = m(x)
    torch.cuda.synchronize()
    assert logp.shape == (2, 399, 11) and logp.is_cuda
    assert torch.allclose(logp.exp().sum(-1).cpu(), torch.ones(2, 399), atol=1e-4)
    assert m.specifications.powerset and m.num_frames(128000) == 399
    e = pipeline._embedding
    assert (e.sample_rate, e.dimension, e.metric) == (16000, 256, "cosine")
    assert e.min_num_samples == 400                               # speaker_verification.py:677-691
    out = e(x[:, :, :32000], torch.ones(2, 99))
    assert out.shape == (2, 256) and np.isfinite(out).all()


def test_from_pretrained_local_hub_dir_vbx(built_lib, gpu, tmp_path):
    """drop-in construction path: a hub directory laid out like BUT-FIT/diarizen-wavlm-*-s80-md
    (config.toml with the REFERENCE class path, pytorch_model.bin = plain state_dict, plda/*.npz) plus
    the WeSpeaker Lightning-style checkpoint ({'state_dict': ...}); VBx clustering branch."""
    import torch as T
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    hub = tmp_path / "hub"
    (hub / "plda").mkdir(parents=True)
    (hub / "wespeaker").mkdir()
    (hub / "config.toml").write_text('''
[model]
path = "diarizen.models.eend.model_wavlm_conformer.Model"
[model.args]
wavlm_src = "wavlm_large_s80_md"
wavlm_layer_num = 25
wavlm_feat_dim = 1024
attention_in = 256
ffn_hidden = 1024
num_head = 4
num_layer = 4
chunk_size = 8
selected_channel = 0
[inference.args]
seg_duration = 8
segmentation_step = 0.1
batch_size = 16
apply_median_filtering = true
[clustering.args]
method = "VBxClustering"
min_speakers = 1
max_speakers = 20
ahc_criterion = "distance"
ahc_threshold = 0.1
Fa = 0.07
Fb = 0.8
lda_dim = 128
max_iters = 20
''')
    cfg = get_seg_config("wavlm_large_s80_md")
    T.save(turn_taking_state_dict(cfg, 0), hub / "pytorch_model.bin")
    T.save({"state_dict": emb_state_dict(0), "pyannote.audio": {"architecture": {"class": "WeSpeakerResNet34"}}},
           hub / "wespeaker" / "pytorch_model.bin")
    g = np.load(os.path.join(GOLD, "host_clustering.npz"))
    for f in ("xvec_transform", "plda"):
        (hub / "plda" / f"{f}.npz").write_bytes(g["plda_" + f].tobytes())
    pipe = DiariZenPipeline.from_pretrained(str(hub), rttm_out_dir=str(tmp_path / "rttm"), device=gpu)
    assert pipe.batch_size == 16 and pipe.apply_median_filtering
    ann = pipe(WAV, sess_name="EN2002a")
    # golden: reference VBxClustering on the oracle's device-stage outputs + oracle/host_stage.py
    assert (tmp_path / "rttm" / "EN2002a.rttm").read_text() == open(os.path.join(GOLD, "e2e_EN2002a_30s_vbx.rttm")).read()
    assert ann.to_rttm().count("SPEAKER EN2002a 1 ") >= 1
    with pytest.raises(Exception):
        DiariZenPipeline.from_pretrained(str(tmp_path / "missing"), cache_dir=str(tmp_path))


def test_der_between_arithmetic_modes(built_lib, gpu):
    """BASELINE configs[4]: the in-tree DER scorer (diarizen_amd/der.py: collar 0, overlap scored, optimal mapping) on the RTTMs
    of the same recording in the three fp32 modes (must be IDENTICAL, DER 0) and in the reduced `f16` mode, which (r5: fp16
    hi*hi + fp8 cross terms, csrc/gemm_mx.hip) is held to SURVEY 8d's reduced bar: |dDER| <= 0.1 abs (percentage points)
    against the fp32 RTTM — on the seeded stress weights, whose margins are far smaller than trained weights'."""
    import copy
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.der import der_rttm
    from diarizen_amd.pipeline import DiariZenPipeline
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    from oracle.gen_golden import E2E_CONFIG
    cfg = get_seg_config("wavlm_large_s80_md")
    rttm = {}
    for prec in ("f32h", "f32s", "f32", "f16"):
        pipe = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision=prec,
                                seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0))
        rttm[prec] = pipe(WAV, sess_name="EN2002a").to_rttm()
        pipe.engine.close()
    gold = open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read()
    for prec in ("f32h", "f32s", "f32"):
        assert rttm[prec] == gold
        assert der_rttm(gold, rttm[prec], "EN2002a")["der"] == 0.0
    d16 = der_rttm(gold, rttm["f16"], "EN2002a")
    print("f16 vs fp32 RTTM on EN2002a_30s (seeded stress weights):", {k: round(v, 4) for k, v in d16.items() if k != "mapping"})
    assert d16["der"] * 100.0 <= 0.1, d16          # SURVEY 8d reduced bar: DER delta <= 0.1 abs
    os.makedirs("gpurun_out", exist_ok=True)
    if os.path.isdir("gpurun_out"):
        import json
        with open("gpurun_out/der_reduced_modes.json", "w") as f:
            json.dump({"reference": "fp32-mode RTTM (== golden)",
                       "f16": {k: v for k, v in d16.items() if k != "mapping"}}, f, indent=1)


def test_streaming_session_equals_offline(pipeline, tmp_path):
    """Row f3: windows scheduled as the audio arrives (pinned ring + copy stream, diarizen_amd/streaming.py).  Feeding the
    fixture in ragged chunks (0.01 s ... 2.9 s, one longer than a ring slot) gives the SAME decisions, embeddings and final
    RTTM as the offline call; provisional annotations appear while audio is still arriving and never run ahead of it."""
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.streaming import StreamingSession, complete_windows
    wave = first_channel_16k(WAV)
    ref = open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read()
    rng = np.random.default_rng(5)
    cuts = [0]
    while cuts[-1] < len(wave):
        cuts.append(min(len(wave), cuts[-1] + int(rng.choice([160, 5000, 16000, 46400, 30001]))))
    chunks = [wave[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    provisional = []
    final = None
    for t, ann in pipeline.stream(chunks, sess_name="EN2002a", refresh_s=4.0, slot_seconds=2.5, slots=3):
        provisional.append((t, ann))
        final = ann
    assert provisional[-1][0] == 30.0 and final.to_rttm() == ref
    assert len(provisional) >= 4                                            # refreshes before the end
    for t, ann in provisional[:-1]:
        assert t < 30.0
        turns = [seg for seg, _ in ann.itertracks()]
        assert turns and max(s.end for s in turns) <= t + 1e-6              # nothing beyond the audio received
    # push form, and the per-window results themselves
    g = np.load(os.path.join(GOLD, "e2e_EN2002a_30s.npz"))
    sess = StreamingSession(pipeline, "EN2002a", refresh_s=None, max_seconds=60.0)
    for c in chunks:
        assert sess.feed(c) is None
        assert sess.done == complete_windows(sess.n, 128000, 12800)
    assert sess.done == 28                                                  # the zero-padded 29th window waits for finish()
    assert sess.finish().to_rttm() == ref
    assert np.array_equal(np.concatenate(sess.seg), g["seg"])
    assert sess.stats["uploads"] >= len(chunks)
    with pytest.raises(RuntimeError):
        sess.feed(chunks[0])


def test_eval_scp_harness_on_the_fixture(built_lib, gpu, tmp_path):
    """BASELINE configs[4] harness (scripts/eval_scp.py = recipes/diar_ssl/infer_avg.py:28-97 + the scoring of
    run_stage.sh:84-91): a Kaldi wav.scp of two sessions (the fixture under two names), the reference RTTM of the set, a
    UEM — one RTTM per session is written and equals the golden, DER is 0 per file and overall, a UEM that drops the second
    half of a session drops its reference speech from the score."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_scp", os.path.join(os.path.dirname(GOLD), "..", "scripts", "eval_scp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gold = open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read()
    scp, ref, uem, out = tmp_path / "wav.scp", tmp_path / "ref.rttm", tmp_path / "all.uem", tmp_path / "out"
    scp.write_text(f"sessA {WAV}\nsessB {WAV}\n")
    ref.write_text(gold.replace("EN2002a", "sessA") + gold.replace("EN2002a", "sessB"))
    uem.write_text("sessA 1 0.000 30.000\nsessB 1 0.000 15.000\n")
    res = mod.main(["-i", str(scp), "-o", str(out), "--ref-rttm", str(ref), "--uem", str(uem), "--synthetic-weights"])
    assert res["recordings"] == 2 and res["der_overall"]["der"] == 0.0
    assert set(res["der_files"]) == {"sessA", "sessB"} and all(f["der"] == 0.0 for f in res["der_files"].values())
    assert (out / "sessA.rttm").read_text() == gold.replace("EN2002a", "sessA")
    assert (out / "sessB.rttm").read_text() == gold.replace("EN2002a", "sessB")
    assert res["der_files"]["sessB"]["total"] < res["der_files"]["sessA"]["total"]       # the UEM cut sessB's scored speech
    assert (out / "result_collar0").exists()


@pytest.mark.parametrize("backends", ["auto", "hip"])
def test_host_stage_30min_device_backends_equal_reference_golden(built_lib, gpu, backends):
    """(r5) the same golden as tests/test_host_ref.py::test_product_host_stage_equals_reference_run_at_30min_scale,
    with the product's DEVICE backends on: centroid linkage on the device (2415 training embeddings >= HIP_LINKAGE_MIN), float64
    cosine scores on the device (8964 rows >= HIP_CDIST_MIN), counting / cluster activations on the device.  `hip` forces them."""
    import json
    from tests._host30 import run_and_check
    res = run_and_check(device=gpu, linkage_backend=backends, cdist_backend=backends)
    print(json.dumps(res))
    os.makedirs("gpurun_out", exist_ok=True)
    json.dump(res, open(f"gpurun_out/host30_{backends}.json", "w"))


def test_diarize_many_overlapped_equals_serial_calls(built_lib, gpu, tmp_path):
    """(r5) the corpus loop of the reference's entry points (diarizen/pipelines/inference.py:365-368) with the
    host stage of recording i in a worker thread beside the device stage of recording i+1: same Annotation / RTTM per recording
    as one `__call__` after the other, in input order, for recordings of different lengths (the host stage's device arena has to
    grow and to be reused), and the golden RTTM of the 30 s fixture.  Also: the host stage's device calls really work on their
    own stream while the default stream is busy."""
    import copy
    import io
    import wave as wave_mod
    from diarizen_amd import _lib, ops
    from diarizen_amd.audio import first_channel_16k
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = get_seg_config("wavlm_large_s80_md")
    pipe = DiariZenPipeline(None, None, config=copy.deepcopy(E2E_CONFIG), device=gpu, precision="f32h",
                            seg_state=turn_taking_state_dict(cfg, 0), emb_state=emb_state_dict(0))
    x = first_channel_16k(WAV)

    def wav_bytes(samples):
        buf = io.BytesIO()
        with wave_mod.open(buf, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.round(np.clip(samples, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
        return buf.getvalue()

    # 30 s, 90 s (the fixture three times with a gain change), 12 s, 30 s again; the first one from its file
    recs = [WAV, wav_bytes(np.concatenate([x, 0.7 * x[::-1], x])), wav_bytes(x[:192000]), wav_bytes(x)]
    names = ["a", "b", "c", "d"]
    serial = [pipe(r, sess_name=n).to_rttm() for r, n in zip(recs, names)]
    assert serial[0] == open(os.path.join(GOLD, "e2e_EN2002a_30s.rttm")).read().replace("EN2002a", "a")
    pipe.rttm_out_dir = str(tmp_path)
    got = list(pipe.diarize_many(recs, sess_names=names, overlap=True))
    assert [n for n, _ in got] == names
    assert [a.to_rttm() for _, a in got] == serial
    assert [(tmp_path / f"{n}.rttm").read_text() for n in names] == serial
    assert len(pipe.corpus_timings) == 4 and all(t["host_s"] > 0 for t in pipe.corpus_timings)
    assert [a.to_rttm() for _, a in pipe.diarize_many(recs, sess_names=names, overlap=False)] == serial
    # the linkage / cdist entry points on their own stream: results while the default stream is kept busy equal the idle ones
    rng = np.random.default_rng(0)
    e = rng.standard_normal((3000, 256)).astype(np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    z_idle = ops.linkage_centroid(e, device=0)
    big = torch.randn(8192, 8192, device=gpu)
    for _ in range(40):
        big = big @ big * 1e-4                      # ~45 ms of queued default-stream work
    z_busy = ops.linkage_centroid(e, device=0)
    torch.cuda.synchronize()
    assert np.array_equal(z_idle, z_busy)
    lib = _lib.load()
    assert lib.dzn_host_workspace_bytes(0) >= 3000 * 3000 * 8
    pipe.close()
    assert lib.dzn_host_workspace_bytes(0) == 0
