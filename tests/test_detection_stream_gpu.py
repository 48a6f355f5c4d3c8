"""Live voice activity / overlapped speech detection (diarizen_amd/detection.py, DetectionStream) on the MI355X: audio fed
in 0.37 s chunks.  After every feed the committed activity and scores only grow and are a prefix of the offline result bit for
bit, every window is computed once, and the final annotation is the offline pipelines' RTTM text — for a recording on the
step grid, one with a zero-padded last window and one shorter than a window."""
import copy

import numpy as np
import pytest

from _stream_cases import RECORDINGS, STEP, WINDOW, feeds, samples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def detectors(built_lib, gpu):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.detection import OverlappedSpeechDetection, VoiceActivityDetection
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    pipe = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield VoiceActivityDetection(pipe), OverlappedSpeechDetection(pipe)
    pipe.close()


_OFFLINE = {}


def offline(detectors, gpu, name):
    """per recording, once: (samples, WAV bytes, offline activity [T, 2], scores [T, 2], VAD RTTM, OSD RTTM)"""
    if name not in _OFFLINE:
        import torch
        from diarizen_amd.inference import window_plan
        from diarizen_amd.postprocess import _frame_grid, crop_end, detect_device, receptive_field
        vad, osd = detectors
        x, data = samples(RECORDINGS[name])
        res = vad._runner.run(torch.from_numpy(x).to(gpu), with_embeddings=False)
        Cn, L, _ = res.segmentations.shape
        grid, _, T = _frame_grid(Cn, L, vad.chunks_window(), receptive_field())
        n_full, has_last = window_plan(len(x), WINDOW, STEP)
        assert (n_full, has_last) == {"grid": (11, False), "padded": (28, True), "short": (0, True)}[name]
        if has_last:
            T = crop_end(T, grid, len(x) / 16000)
        act, sc, _ = detect_device(res.segmentations, vad.chunks_window(), receptive_field(), 3, num_frames=T, want_scores=True)
        file = {"audio": data, "uri": name}
        act.setflags(write=False)
        sc.setflags(write=False)
        _OFFLINE[name] = (x, data, act, sc, vad(file).to_rttm(), osd(file).to_rttm())
    return _OFFLINE[name]


def lines(rttm, label):
    return "".join(ln + "\n" for ln in rttm.splitlines() if f" {label} " in ln)


@pytest.mark.parametrize("name", list(RECORDINGS))
def test_committed_prefix_after_every_feed_and_final_result(detectors, gpu, name):
    """both detections from one pass (tasks = 3): the per-feed properties, then the final annotation against vad(wav) and
    osd(wav) label by label"""
    from diarizen_amd.streaming import complete_windows
    vad, _ = detectors
    x, _, act, sc, vad_rttm, osd_rttm = offline(detectors, gpu, name)
    sess = vad.open_stream(uri=name, tasks=3, scores=True, max_seconds=60.0, slot_seconds=2.5, slots=3)
    assert sess.labels == ["SPEECH", "OVERLAP"]
    prev_a, prev_s = np.zeros((0, 2), np.uint8), np.zeros((0, 2), np.float32)
    seen = 0
    for c in feeds(x):
        ann = sess.feed(c)
        done = complete_windows(sess.n, WINDOW, STEP)
        assert sess.done == done == sess.stats["windows"]                     # each window once, as soon as it is complete
        a, s = sess.committed_activity, sess.committed_scores
        F = len(a)
        assert a.dtype == np.uint8 and s.dtype == np.float32 and a.shape == s.shape == (F, 2)
        assert F >= len(prev_a) and np.array_equal(a[:len(prev_a)], prev_a)
        assert np.array_equal(s[:len(prev_s)].view(np.uint32), prev_s.view(np.uint32))
        assert F <= len(act) and np.array_equal(a, act[:F])
        assert np.array_equal(s.view(np.uint32), sc[:F].view(np.uint32))
        assert F == (0 if done == 0 else round(done * STEP / 320))            # the start frame of the next window
        assert sess.committed_seconds == pytest.approx(F * 0.02) and sess.seconds == sess.n / 16000
        if done == 0:
            assert ann is None
        else:
            assert ann is not None and ann.uri == name
            turns = list(ann.itertracks(yield_label=True))
            assert {lab for _, _, lab in turns} <= {"SPEECH", "OVERLAP"}
            # nothing beyond the audio received: regions end at frame middles, and the last frame of a window that the
            # newest sample completes is centred half a frame duration (12.5 ms) behind it, as offline
            assert all(seg.end <= sess.seconds + 0.0125 + 1e-6 for seg, _, _ in turns)
            seen += 1
        prev_a, prev_s = a, s
    if name == "short":
        assert seen == 0 and len(prev_a) == 0
    else:
        assert seen > 10 and 0 < len(prev_a) < len(act)
    final = sess.finish()
    assert sess.stats["windows"] == sess.done == {"grid": 11, "padded": 29, "short": 1}[name]
    assert sess.stats["range_calls"] <= sess.stats["launches"] + 1 and sess.stats["uploads"] >= len(feeds(x))
    assert np.array_equal(sess.committed_activity, act)
    assert np.array_equal(sess.committed_scores.view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(sess.committed_activity[:len(prev_a)], prev_a)
    rttm = final.to_rttm()
    assert lines(rttm, "SPEECH") == vad_rttm and lines(rttm, "OVERLAP") == osd_rttm
    assert len(rttm.splitlines()) == len(vad_rttm.splitlines()) + len(osd_rttm.splitlines())
    with pytest.raises(RuntimeError):
        sess.feed(x[:10])


@pytest.mark.parametrize("name", list(RECORDINGS))
def test_generator_form_gives_the_offline_rttm_text(detectors, gpu, name, tmp_path):
    """vad.stream / osd.stream: (seconds, committed seconds, Annotation) per feed that has one, the last triple is the
    offline call's RTTM text; the RTTM file lands in rttm_out_dir"""
    x, _, act, _, vad_rttm, osd_rttm = offline(detectors, gpu, name)
    for det, ref in zip(detectors, (vad_rttm, osd_rttm)):
        det.rttm_out_dir = str(tmp_path)
        try:
            out = list(det.stream(feeds(x), uri=name, max_seconds=60.0))
        finally:
            det.rttm_out_dir = None
        secs, committed, ann = out[-1]
        assert secs == len(x) / 16000 and committed == pytest.approx(len(act) * 0.02)
        assert ann.to_rttm() == ref
        assert (tmp_path / f"{name}.rttm").read_text() == ref
        assert [t[0] for t in out] == sorted(t[0] for t in out) and [t[1] for t in out] == sorted(t[1] for t in out)
        assert all(c <= s for s, c, _ in out[:-1])
        assert len(out) == 1 if name == "short" else len(out) > 10


def test_duration_parameters_final_rttm_equals_offline(detectors, gpu):
    """min_duration_off / min_duration_on: the final annotation gets Binarize's post-processing as apply() does (and the
    provisional ones on the way)"""
    x, data, _, _, vad_rttm, osd_rttm = offline(detectors, gpu, "padded")
    for det, base in zip(detectors, (vad_rttm, osd_rttm)):
        det.instantiate({"min_duration_on": 0.5, "min_duration_off": 0.3})
        try:
            ref = det({"audio": data, "uri": "padded"}).to_rttm()
            out = list(det.stream(feeds(x), uri="padded", max_seconds=60.0))
        finally:
            det.instantiate(det.default_parameters())
        assert ref != base                                                    # the parameters change this recording's regions
        assert out[-1][2].to_rttm() == ref
        assert all(seg.duration >= 0.5 for _, _, ann in out for seg, _ in ann.itertracks())


def test_refuses_distributed_runs_and_bad_task_masks(detectors, gpu, monkeypatch):
    vad, _ = detectors
    with pytest.raises(ValueError):
        vad.open_stream(tasks=4)
    monkeypatch.setattr("diarizen_amd.dist.world_size", lambda: 2)
    with pytest.raises(RuntimeError):
        vad.open_stream(uri="x")
