"""Online speaker assignment: global speaker labels for the local speakers of one window at a time, never revised
(the host half of live.LiveDiarization; pure numpy float64, needs no device).

Offline, the pipeline clusters the embeddings of ALL windows (centroid-linkage AHC cut at `ahc_threshold`, then a Hungarian
assignment of every window's local speakers to the centroids, clustering.py).  Online there is no "all": each window is
labelled when it arrives, against the centroids of the speakers met so far —

    d[s, k] = || x_s - sums[k] / n[k] ||_2,     x_s = emb_s / ||emb_s||_2

the distance centroid linkage thresholds on L2-normalised embeddings, so `delta_new` lives on the scale of `ahc_threshold`.

  phase 1   Hungarian assignment (scipy linear_sum_assignment) of the window's candidates to the existing speakers; a matched
            pair with d <= delta_new is accepted
  phase 2   the other candidates in ascending s: a CLEAN one (enough frames in which it is the only active speaker, the rule
            of clustering.filter_embeddings) opens the next speaker while fewer than max_speakers exist — labels are numbered
            by first appearance; otherwise it is forced to the nearest existing speaker that no local speaker of this window
            holds, and gets -2 when none is free.  A non-clean embedding (mostly overlapped speech) never opens a speaker
  update    after both phases: accepted pairs whose local speaker is clean add x_s to their speaker's sum, a new speaker
            starts with x_s; forced assignments and non-clean embeddings never move a centroid

min_cluster_size is not applied — a cluster's size is only known at the end — so a spurious small speaker is possible until
LiveDiarization.finish(recluster=True)."""
from __future__ import annotations

import numpy as np

from .clustering import active_speakers, single_speaker_frame_mask


class OnlineSpeakers:
    def __init__(self, delta_new: float, max_speakers: int, dim: int = 256):
        self.delta_new = float(delta_new)
        self.max_speakers = int(max_speakers)
        self.sums = np.zeros((0, int(dim)), dtype=np.float64)        # per speaker: sum of its L2-normalised member embeddings
        self.n = np.zeros(0, dtype=np.int64)                         # ... and their number

    @property
    def num_speakers(self) -> int:
        return len(self.n)

    @property
    def centroids(self) -> np.ndarray:
        return self.sums / self.n[:, None]

    def assign(self, seg_c: np.ndarray, emb_c: np.ndarray) -> np.ndarray:
        """seg_c [L, S] decisions of one window, emb_c [S, D] its embeddings -> int8 [S] global labels (-2: inactive, NaN
        embedding, or no label free).  Call once per window, in window order."""
        seg = np.asarray(seg_c)[None]
        L, S = seg.shape[1:]
        active = active_speakers(seg)[0]
        clean = single_speaker_frame_mask(seg, round(0.1 * L))[0]
        emb = np.asarray(emb_c, dtype=np.float64)
        out = np.full(S, -2, dtype=np.int8)
        cand = np.nonzero(active & ~np.isnan(emb).any(axis=1))[0]
        if len(cand) == 0:
            return out
        norm = np.linalg.norm(emb[cand], axis=1, keepdims=True)
        x = emb[cand] / np.where(norm > 0.0, norm, 1.0)              # an all-zero embedding stays the origin
        K = self.num_speakers
        d = np.linalg.norm(x[:, None, :] - self.centroids[None, :, :], axis=2) if K else np.zeros((len(cand), 0))
        taken = np.zeros(K, dtype=bool)
        members, opened = [], []                                     # (speaker, candidate index) whose x moves / starts a centroid
        if K:
            from scipy.optimize import linear_sum_assignment
            for i, k in zip(*linear_sum_assignment(d)):
                if d[i, k] <= self.delta_new:
                    out[cand[i]] = k
                    taken[k] = True
                    if clean[cand[i]]:
                        members.append((k, i))
        for i, s in enumerate(cand):
            if out[s] >= 0:
                continue
            if clean[s] and K + len(opened) < self.max_speakers:
                out[s] = K + len(opened)
                opened.append(i)
            elif not taken.all():
                k = int(np.argmin(np.where(taken, np.inf, d[i])))
                out[s] = k
                taken[k] = True
        for k, i in members:
            self.sums[k] += x[i]
            self.n[k] += 1
        if opened:
            self.sums = np.concatenate([self.sums, x[opened]])
            self.n = np.concatenate([self.n, np.ones(len(opened), dtype=np.int64)])
        return out
