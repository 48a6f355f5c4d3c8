"""online.OnlineSpeakers on the CPU: known answers on hand-built windows (every branch of the two phases and of the centroid
update), planted clean speakers (labels are a bijection with the identities), and oracle.gen_golden.synth_host_case — overlaps,
and non-clean speakers that appear before their centroid exists — within 4 % of the nearest planted prototype."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from diarizen_amd.online import OnlineSpeakers

L, S, D = 20, 3, 4                  # clean = at least round(0.1 * 20) = 2 frames alone
E = np.eye(D, dtype=np.float32)


def win(spans):
    """{local speaker: (first frame, end frame)} -> u8 [L, S]"""
    seg = np.zeros((L, S), dtype=np.uint8)
    for s, (a, b) in spans.items():
        seg[a:b, s] = 1
    return seg


def emb(*rows):
    out = np.zeros((S, D), dtype=np.float32)
    for s, r in enumerate(rows):
        out[s] = r
    return out


def unit(*v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def two_speakers(delta, cap=20):
    """speakers 0 and 1 with centroids e0 and e1"""
    o = OnlineSpeakers(delta, cap, dim=D)
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(E[0], E[1])).tolist() == [0, 1, -2]
    return o


def test_inactive_and_nan_local_speakers_get_minus_two():
    o = OnlineSpeakers(0.5, 20, dim=D)
    out = o.assign(win({0: (0, 10), 2: (10, 20)}), emb(3 * E[0], E[1], [np.nan, 0, 0, 0]))
    assert out.dtype == np.int8 and out.tolist() == [0, -2, -2]
    assert o.num_speakers == 1 and np.array_equal(o.sums, E[:1]) and o.n.tolist() == [1]      # the sum holds emb / |emb|


def test_labels_are_numbered_by_first_appearance():
    o = OnlineSpeakers(0.5, 20, dim=D)
    assert o.assign(win({0: (0, 8), 2: (10, 18)}), emb(E[0], 0, E[1])).tolist() == [0, -2, 1]
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(E[2], E[1], 0)).tolist() == [2, 1, -2]
    assert o.assign(win({1: (3, 9)}), emb(0, E[0], 0)).tolist() == [-2, 0, -2]
    assert o.num_speakers == 3 and o.n.tolist() == [2, 2, 1]


def test_within_delta_joins_and_moves_the_centroid_beyond_it_a_clean_speaker_opens_a_label():
    o = two_speakers(0.5)
    near, far = unit(1, 0.3, 0, 0), unit(1, 0, 1, 0)            # 0.29 and 0.77 from e0
    assert np.linalg.norm(near - E[0]) < 0.5 < np.linalg.norm(far - E[0])
    assert o.assign(win({1: (0, 9)}), emb(0, 5 * near, 0)).tolist() == [-2, 0, -2]
    assert o.n.tolist() == [2, 1] and np.allclose(o.sums[0], E[0] + near, rtol=0, atol=1e-7)
    # the distance is to the CENTROID (sums / n), and exactly at delta_new the pair is still accepted
    c0 = o.centroids[0]
    o.delta_new = float(np.linalg.norm(unit(1, 0.6, 0, 0) - c0))
    assert o.assign(win({2: (0, 9)}), emb(0, 0, unit(1, 0.6, 0, 0))).tolist() == [-2, -2, 0]
    o.delta_new = 0.5
    assert o.assign(win({0: (0, 9)}), emb(far, 0, 0)).tolist() == [2, -2, -2]
    assert o.num_speakers == 3 and np.allclose(o.sums[2], far, rtol=0, atol=1e-7)


def test_non_clean_speakers_are_forced_to_distinct_nearest_labels_and_move_no_centroid():
    o = two_speakers(0.1)
    before = (o.sums.copy(), o.n.copy())
    # both local speakers are active in the same frames only (no frame alone), both nearest e1 and beyond delta_new of it
    out = o.assign(win({0: (2, 12), 1: (2, 12)}), emb(unit(0.5, 1, 0, 0), unit(0.4, 1, 0, 0), 0))
    assert out.tolist() == [1, 0, -2]                           # ascending s: s = 0 takes the nearest, s = 1 the one left
    assert o.num_speakers == 2 and np.array_equal(o.sums, before[0]) and np.array_equal(o.n, before[1])
    # a non-clean speaker WITHIN delta_new is accepted by the matching, and still moves nothing
    assert o.assign(win({0: (2, 12), 1: (2, 12)}), emb(unit(0.01, 1, 0, 0), unit(1, 0.01, 0, 0), 0)).tolist() == [1, 0, -2]
    assert np.array_equal(o.sums, before[0]) and np.array_equal(o.n, before[1])


def test_a_non_clean_speaker_never_opens_a_label():
    o = OnlineSpeakers(0.5, 20, dim=D)
    assert o.assign(win({0: (2, 12), 1: (2, 13)}), emb(E[0], E[1], 0)).tolist() == [-2, -2, -2]       # s = 1 is alone in 1 frame
    assert o.num_speakers == 0
    assert o.assign(win({0: (2, 12), 1: (2, 14)}), emb(E[0], E[1], 0)).tolist() == [-2, 0, -2]        # ... in 2 frames: clean
    assert o.num_speakers == 1


def test_two_clean_speakers_nearest_the_same_centroid_get_distinct_labels():
    o = two_speakers(0.5)
    a, b = unit(1, 0.1, 0, 0), unit(1, 0.2, 0, 0)               # both nearest e0 and within delta_new of it
    assert max(np.linalg.norm(a - E[0]), np.linalg.norm(b - E[0])) < 0.5
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(a, b, 0)).tolist() == [0, 2, -2]       # the matching gives e0 once
    assert o.num_speakers == 3 and o.n.tolist() == [2, 1, 1]


def test_at_the_cap_nothing_new_opens_and_with_nothing_free_the_label_is_minus_two():
    a, b = unit(1, 0.1, 0, 0), unit(1, 0.2, 0, 0)
    o = two_speakers(0.5, cap=2)
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(a, b, 0)).tolist() == [0, 1, -2]       # forced to the free label 1
    assert o.num_speakers == 2 and o.n.tolist() == [2, 1] and np.array_equal(o.sums[1], E[1])
    o = OnlineSpeakers(0.5, 1, dim=D)
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(E[0], E[1], 0)).tolist() == [0, -2, -2]      # the cap holds in one window
    assert o.assign(win({0: (0, 8), 1: (10, 18)}), emb(b, a, 0)).tolist() == [-2, 0, -2]      # the nearer one is matched
    assert o.assign(win({2: (0, 8)}), emb(0, 0, E[2])).tolist() == [-2, -2, 0]                # beyond delta_new, clean, forced
    assert o.num_speakers == 1 and o.n.tolist() == [2]


def test_planted_clean_speakers_give_a_bijection():
    g = np.random.default_rng(11)
    n_spk, C, Lw, Sw, Dw = 5, 80, 99, 4, 256
    protos = g.normal(size=(n_spk, Dw))
    o = OnlineSpeakers(0.8, 20, dim=Dw)
    pairs = set()
    for _ in range(C):
        k = int(g.integers(1, 4))
        who, slots = g.permutation(n_spk)[:k], g.permutation(Sw)[:k]
        cuts = np.linspace(0, Lw, k + 1).astype(int)
        seg, e = np.zeros((Lw, Sw), np.uint8), (0.1 * g.normal(size=(Sw, Dw))).astype(np.float32)
        for i, (spk, slot) in enumerate(zip(who, slots)):
            seg[cuts[i] + int(g.integers(0, 5)):cuts[i + 1] - int(g.integers(0, 5)), slot] = 1
            e[slot] = protos[spk] + 0.35 * g.normal(size=Dw)
        out = o.assign(seg, e)
        assert all(out[s] == -2 for s in range(Sw) if s not in slots)
        pairs.update((int(out[slot]), int(spk)) for spk, slot in zip(who, slots))
    assert o.num_speakers == n_spk and len(pairs) == n_spk
    assert sorted(p[0] for p in pairs) == sorted(p[1] for p in pairs) == list(range(n_spk))


@pytest.mark.parametrize("seed,C,n_spk", [(1, 60, 3), (2, 60, 4), (3, 120, 6), (4, 30, 2), (5, 200, 5)])
def test_synth_host_case_speaker_count_and_labels(seed, C, n_spk):
    from oracle.gen_golden import synth_host_case
    seg, e = synth_host_case(seed, C=C, n_spk=n_spk)
    protos = np.random.default_rng(seed).normal(size=(n_spk, e.shape[2]))        # the generator's first draw
    o = OnlineSpeakers(0.8, 20, dim=e.shape[2])
    lab = np.stack([o.assign(seg[c], e[c]) for c in range(C)])
    assert o.num_speakers == n_spk
    active = seg.sum(axis=1) > 0
    assert (lab[~active] == -2).all()
    x = e / np.linalg.norm(e, axis=2, keepdims=True)
    truth = np.argmax(x @ (protos / np.linalg.norm(protos, axis=1, keepdims=True)).T, axis=2)
    conf = np.zeros((n_spk, n_spk), dtype=np.int64)
    for l, t in zip(lab[active], truth[active]):
        if l >= 0:
            conf[l, t] += 1
    r, c = linear_sum_assignment(-conf)                                         # the best label matching
    wrong = 1.0 - conf[r, c].sum() / active.sum()
    print(f"seed {seed}: {active.sum()} active entries, {wrong:.2%} not on the nearest planted prototype")
    assert wrong <= 0.04
