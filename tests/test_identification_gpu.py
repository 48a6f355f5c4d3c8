"""Speaker identification end to end on the MI355X (diarizen_amd/identification.py over csrc/gallery.hip): the seeded pipeline
of tests/test_live_diarization_gpu.py on the "padded" 30 s recording of tests/_stream_cases.py.  return_embeddings hands out
the clustering's centroids without changing the diarization, voiceprint picks the dominant label's row, a gallery of the
recording's own centroids among 100 distractors names every label, the rule is exclusive, and live sessions are identified with
one search for all of them."""
import copy

import numpy as np
import pytest

from _gallery_cases import bound
from _stream_cases import RECORDINGS, samples

DELTA = 0.2                                         # the seeded embedding weights: 3 speakers at 0.2
KW = dict(delta_new=DELTA, max_seconds=60.0, slot_seconds=2.5, slots=3)
FEED_LONG = 46400                                   # 2.9 s per feed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(built_lib, gpu):
    from diarizen_amd.configs import get_seg_config
    from diarizen_amd.pipeline import DiariZenPipeline
    from oracle.gen_golden import E2E_CONFIG
    from testkit.weights import emb_state_dict, turn_taking_state_dict
    cfg = copy.deepcopy(E2E_CONFIG)
    cfg["inference"]["args"]["batch_size"] = 64
    p = DiariZenPipeline(None, None, config=cfg, device=gpu, seg_state=turn_taking_state_dict(get_seg_config(
        "wavlm_large_s80_md"), 0), emb_state=emb_state_dict(0))
    yield p
    p.close()


@pytest.fixture(scope="module")
def base(pipe):
    """once: (samples, WAV bytes, the plain call's RTTM, the clustering's centroids computed from device_stage's output)"""
    x, data = samples(RECORDINGS["padded"])
    rttm = pipe(data, sess_name="padded").to_rttm()
    seg, emb = pipe.device_stage(x)
    cent = pipe.clustering(embeddings=emb, segmentations=seg, min_clusters=pipe.min_speakers, max_clusters=pipe.max_speakers)[2]
    cent = np.asarray(cent)
    cent.setflags(write=False)
    assert len({ln.split()[7] for ln in rttm.splitlines()}) >= 2
    return x, data, rttm, cent


@pytest.fixture(scope="module")
def gallery(base, gpu):
    """the recording's own centroids as spk0, spk1, ... among 100 seeded random distractors"""
    from diarizen_amd.identification import SpeakerGallery
    cent = base[3]
    g = SpeakerGallery(256, gpu, capacity=64)
    noise = np.random.default_rng(5).standard_normal((100, 256), dtype=np.float32)
    for i in range(50):
        g.enroll(f"other{i}", noise[i])
    for k in range(len(cent)):
        g.enroll(f"spk{k}", cent[k])
    for i in range(50, 100):
        g.enroll(f"other{i}", noise[i])
    yield g
    g.close()


def substituted(rttm: str, names: dict) -> str:
    out = []
    for line in rttm.splitlines():
        f = line.split(" ")
        f[7] = names.get(int(f[7]), f[7])
        out.append(" ".join(f) + "\n")
    return "".join(out)


def test_return_embeddings_are_the_centroids_and_change_nothing(pipe, base):
    _, data, rttm, cent = base
    out = pipe(data, sess_name="padded", return_embeddings=True)
    assert isinstance(out, tuple) and len(out) == 2
    ann, emb = out
    assert ann.to_rttm() == rttm
    K = len(cent)
    assert emb.dtype == np.float32 and emb.shape == (K, 256)
    assert np.array_equal(emb.view(np.uint32), cent.astype(np.float32).view(np.uint32))
    assert max(int(ln.split()[7]) for ln in rttm.splitlines()) < K                      # row k = label k
    ann_s, scores = pipe(data, sess_name="padded", return_scores=True)
    ann3, scores3, emb3 = pipe(data, sess_name="padded", return_scores=True, return_embeddings=True)
    assert ann3.to_rttm() == ann_s.to_rttm() == rttm and np.array_equal(scores3.data, scores.data)
    assert np.array_equal(emb3, emb) and scores3.data.shape[1] <= K


def test_voiceprint_is_the_row_of_the_label_with_the_most_speech(pipe, base):
    _, data, rttm, cent = base
    total = {}
    for ln in rttm.splitlines():
        f = ln.split()
        total[int(f[7])] = total.get(int(f[7]), 0.0) + float(f[4])
    best = min(total, key=lambda k: (-total[k], k))
    assert sorted(total.values())[-1] - sorted(total.values())[-2] > 0.01               # (no tie hidden by the RTTM's 3 digits)
    v = pipe.voiceprint(data)
    assert v.dtype == np.float32 and v.shape == (256,) and np.array_equal(v, cent[best].astype(np.float32))


def test_every_label_is_named_among_distractors(pipe, base, gallery):
    from diarizen_amd.identification import SpeakerIdentification
    _, data, rttm, cent = base
    ident = SpeakerIdentification(pipe, gallery, threshold=0.5)
    ann, ids = ident(data, sess_name="padded")
    assert [i.label for i in ids] == list(range(len(cent)))
    for i in ids:
        print(f"label {i.label}: {i.name} {i.score:.7f}, runner-up {i.runner_up} {i.runner_up_score:.7f}")
        assert i.name == f"spk{i.label}" and i.score >= 1.0 - bound(256)
        assert i.runner_up is not None and i.runner_up != i.name and i.runner_up_score <= i.score
    assert ann.to_rttm() == substituted(rttm, {k: f"spk{k}" for k in range(len(cent))}) and ann.uri == "padded"
    with pytest.raises(TypeError):
        SpeakerIdentification(pipe, gallery)                                            # the threshold has no default


def test_a_threshold_above_one_names_nobody(pipe, base, gallery):
    from diarizen_amd.identification import SpeakerIdentification
    _, data, rttm, _ = base
    ann, ids = SpeakerIdentification(pipe, gallery, threshold=1.5)(data, sess_name="padded")
    assert all(i.name is None and i.score is None and i.runner_up is not None for i in ids)
    assert ann.to_rttm() == rttm


def test_one_enrolled_speaker_names_exactly_one_label(pipe, base, gpu):
    """the seeded embedding weights put the speakers close together: every label scores high against speaker 0's voiceprint,
    and a rule that is not one-to-one would name several"""
    from diarizen_amd.identification import SpeakerGallery, SpeakerIdentification
    _, data, rttm, cent = base
    g = SpeakerGallery(256, gpu, capacity=8)
    try:
        g.enroll("zero", cent[0])
        threshold = 0.0
        scores, _ = g.search(cent, 1)
        print("cosine of every centroid to speaker 0's:", scores[:, 0])
        ann, ids = SpeakerIdentification(pipe, g, threshold=threshold)(data, sess_name="padded")
        assert [i.name for i in ids] == ["zero"] + [None] * (len(cent) - 1)
        assert ann.to_rttm() == substituted(rttm, {0: "zero"})
        if len(cent) > 1:
            assert (scores[1:, 0] >= threshold).any()          # ... so exclusivity, not the threshold, kept the others unnamed
    finally:
        g.close()


def _identities(gallery, centroids, threshold):
    """the rule restated: one search of the centroids, assign_identities, names"""
    from diarizen_amd.identification import assign_identities
    c = np.asarray(centroids, dtype=np.float32)
    scores, slots = gallery.search_slots(c, min(len(c), len(gallery)))
    matched = assign_identities(scores, slots, threshold)
    out = []
    for k, m in enumerate(matched):
        score = None if m is None else float(scores[k][list(slots[k]).index(m)])
        out.append((k, None if m is None else gallery._name[m], score))
    return out


def test_live_sessions_are_identified_with_one_search(pipe, base, gallery):
    from diarizen_amd.identification import SpeakerIdentification
    x = base[0]
    ident = SpeakerIdentification(pipe, gallery, threshold=0.5)
    sess = pipe.open_live(sess_name="solo", **KW)
    for i in range(0, len(x), FEED_LONG):
        sess.feed(x[i:i + FEED_LONG])
    cent = sess.centroids
    assert cent.shape == (sess.num_speakers, 256) and sess.num_speakers >= 1
    cent[:] = 0.0
    assert np.abs(sess.centroids).sum() > 0                                             # a copy
    labels_before = sess.hard_clusters
    got = ident.identify_live([sess])
    assert list(got) == ["solo"]
    assert [(i.label, i.name, i.score) for i in got["solo"]] == _identities(gallery, sess.centroids, 0.5)
    assert np.array_equal(sess.hard_clusters, labels_before)                            # live labels are not renamed
    sess.finish()

    hub = pipe.open_hub(max_sessions=2, max_seconds=60.0)
    try:
        a, b = hub.open("a", delta_new=DELTA), hub.open("b", delta_new=DELTA)
        xa, xb = x[:20 * 16000], x[10 * 16000:24 * 16000]
        for i in range(0, len(xa), FEED_LONG):
            a.feed(xa[i:i + FEED_LONG])
            if i < len(xb):
                b.feed(xb[i:i + FEED_LONG])
            hub.tick()
        assert a.num_speakers >= 1 and b.num_speakers >= 1
        before = gallery.searches
        got = ident.identify_live(hub.sessions.values())
        assert gallery.searches == before + 1                                           # ONE search for both sessions
        assert sorted(got) == ["a", "b"]
        for s in (a, b):
            assert [(i.label, i.name, i.score) for i in got[s.name]] == _identities(gallery, s.centroids, 0.5)
            assert [(i.label, i.name, i.score) for i in ident.identify_live([s])[s.name]] == \
                [(i.label, i.name, i.score) for i in got[s.name]]
        a.finish()
        b.finish()
        hub.tick()
    finally:
        hub.close()
