"""Linking speakers across recordings: is Monday's speaker 2 Tuesday's speaker 0?

No reference counterpart: the reference (and every pipeline here) ends at labels that restart at 0 in each recording.
`identification.py` names speakers who were enrolled beforehand; this module is the unsupervised, order-independent case —
nobody is enrolled, the corpus itself defines the people.  The voiceprints are the cluster centroids the engine already
produces (`__call__(return_embeddings=True)`, `diarize_many(return_embeddings=True)`, `LiveDiarization.centroids`).

The rule is complete-linkage agglomerative clustering of all voiceprints of the corpus on cosine distance, cut at a
threshold, under a cannot-link constraint: two labels of one recording are different people.  As three lines of scipy:

    y = pdist(E.astype(float64), "cosine")
    y[pairs of one recording] = BIG          # 4.0: finite, above every cosine distance (<= 2)
    Z = linkage(y, "complete");  fcluster(Z, threshold, "distance")

With complete linkage the distance of two clusters is the max over their member pairs, so one forbidden pair keeps every union
that would hold it above any threshold in (0, 2]: no constrained data structure is needed.  The same max gives the guarantee
`SpeakerLinks.diameter` states: any two voiceprints of an identity are at most that far apart.

  SpeakerLinker   add(recording, voiceprints) per recording, then link() once -> SpeakerLinks
  SpeakerLinks    identity[(recording, label)], members, diameter, relabel / names

backend "scipy" is the definition above; "hip" is csrc/linkage.hip (dzn_link_speakers: the float64 matrix resident in HBM, the
step loop of the centroid linkage with the max update, stopped at the threshold) and a union-find over the merges it returns.

The threshold is required and has no default: a cosine operating point can only come from real checkpoints and real speakers,
and nothing here can calibrate one (seeded weights only)."""
from __future__ import annotations

from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np

from . import clustering
from .identification import _device_index, _usable
from .identification import relabel as _relabel

BIG = 4.0      # the distance of a forbidden pair (csrc/linkage.hip: LINK_BIG)

# "auto" takes the device from this many usable voiceprints up.  Measured on one idle MI355X (scripts/link_timing.py ->
# profiles/link_timing.json, dim 256): the device call and scipy's pdist + linkage meet at n = 512 (6.4 ms against 6.0 ms) and
# the device is 2.2x ahead at 1024 (12.2 against 27.3 ms), 19x at 8192; 1024 leaves that factor for a device that is busy with
# a pipeline's windows.
HIP_LINK_MIN = 1024


def masked_cosine_pdist(emb: np.ndarray, group: np.ndarray) -> np.ndarray:
    """the condensed float64 cosine distances of the rows, BIG where two rows share a group"""
    from scipy.spatial.distance import pdist
    y = pdist(np.asarray(emb).astype(np.float64), "cosine")
    i, j = np.triu_indices(len(emb), 1)
    g = np.asarray(group)
    y[g[i] == g[j]] = BIG
    return y


def link_scipy(emb: np.ndarray, group: np.ndarray, threshold: float) -> Tuple[np.ndarray, int]:
    """the definition: (the complete-linkage dendrogram of the masked distances, the number of its merges <= threshold)"""
    from scipy.cluster.hierarchy import linkage
    Z = linkage(masked_cosine_pdist(emb, group), "complete")
    return Z, int(np.count_nonzero(Z[:, 2] <= threshold))


def _union_find(n: int, merges: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """merges: rows of a scipy dendrogram in order (ids < n are rows, n + k is the cluster of merge k) -> (root int [n] of every
    row, height float [n]: per root the height of its last merge, 0.0 for a singleton)"""
    parent = np.arange(n)
    top = list(range(n))            # dendrogram id -> a row of that cluster
    height = np.zeros(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, h, _ in merges:
        ra, rb = find(top[int(a)]), find(top[int(b)])
        parent[rb] = ra
        height[ra] = h
        top.append(ra)
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    return root, height


class SpeakerLinks:
    """The result of SpeakerLinker.link().
      identity        {(recording, label): int}; identities are numbered by first appearance in `add` order (then row order),
                      so the numbers do not depend on cluster ids or on the backend
      unusable        [(recording, label)] whose voiceprint is all zero or not finite: kept out of the clustering, each with an
                      identity of its own
      diameter        {identity: float}: the height of the identity's last merge, 0.0 for a singleton — with complete linkage
                      every two voiceprints of the identity are at most this far apart (cosine distance)
      num_identities  len(diameter)
      backend         "scipy", "hip" or "trivial" (fewer than two usable voiceprints): what computed it"""

    def __init__(self, keys: Sequence[Tuple[Hashable, Hashable]], ids: Sequence[int], diameter: Dict[int, float],
                 unusable: Sequence[Tuple[Hashable, Hashable]], threshold: float, backend: str):
        self.identity: Dict[Tuple[Hashable, Hashable], int] = {k: int(i) for k, i in zip(keys, ids)}
        self.diameter = dict(diameter)
        self.unusable = list(unusable)
        self.threshold, self.backend = float(threshold), backend
        self._members: Dict[int, list] = {i: [] for i in self.diameter}
        for k, i in zip(keys, ids):
            self._members[int(i)].append(k)

    @property
    def num_identities(self) -> int:
        return len(self.diameter)

    def members(self, identity: int) -> List[Tuple[Hashable, Hashable]]:
        """the (recording, label) pairs of one identity, in `add` order"""
        return list(self._members[int(identity)])

    def names(self, recording, fmt: str = "spk{:04d}") -> Dict:
        """{label of `recording`: fmt.format(identity)}"""
        return {label: fmt.format(i) for (rec, label), i in self.identity.items() if rec == recording}

    def relabel(self, recording, annotation, fmt: str = "spk{:04d}"):
        """the annotation of `recording` with its labels replaced by the corpus-wide names (identification.relabel)"""
        return _relabel(annotation, self.names(recording, fmt))


class SpeakerLinker:
    def __init__(self, threshold: float, dim: int = 256, device=None, backend: str = "auto"):
        """threshold: the cosine DISTANCE (1 - cosine) up to which two clusters of voiceprints merge, in (0, 2].  Required, no
        default: nothing here can calibrate one (seeded weights only).  device: a torch.device, an
        ordinal or None (the current device).  backend: "scipy", "hip" (raises when the device path fails) or "auto": the
        device from HIP_LINK_MIN usable voiceprints up when a device and the library are present, scipy when two usable rows
        are bit-identical (exact ties: scipy's order and the device's lowest-index rule may differ, as
        clustering.centroid_linkage) or when the device call fails (e.g. the n x n matrix does not fit)."""
        threshold = float(threshold)
        if not (0.0 < threshold <= 2.0):
            raise ValueError(f"threshold is a cosine distance in (0, 2], not {threshold!r}")
        if backend not in ("auto", "scipy", "hip"):
            raise ValueError(f"unknown linking backend {backend!r}")
        if int(dim) < 1:
            raise ValueError(f"dim must be at least 1, not {dim!r}")
        self.threshold, self.dim, self.device, self.backend = threshold, int(dim), device, backend
        self._recordings: List[Hashable] = []
        self._rows: List[np.ndarray] = []
        self._labels: List[list] = []
        self.device_calls = 0             # library calls made (ops.link_speakers)

    def __len__(self) -> int:
        return sum(len(r) for r in self._rows)

    def add(self, recording, voiceprints, labels: Optional[Sequence] = None) -> None:
        """the K voiceprints of one recording: float32 [K, dim] (row k = label k unless `labels` names them), or a
        live.LiveDiarization (its `centroids`).  K = 0 is allowed; a recording name can be added once."""
        if recording in self._recordings:
            raise ValueError(f"recording {recording!r} was added before")
        rows = getattr(voiceprints, "centroids", voiceprints)
        rows = np.array(rows, dtype=np.float32, copy=True).reshape(-1, self.dim) if np.size(rows) else \
            np.zeros((0, self.dim), dtype=np.float32)
        labels = list(range(len(rows))) if labels is None else list(labels)
        if len(labels) != len(rows) or len(set(labels)) != len(labels):
            raise ValueError(f"{recording!r}: one distinct label per voiceprint ({len(rows)} rows, labels {labels!r})")
        self._recordings.append(recording)
        self._rows.append(rows)
        self._labels.append(labels)

    def _merges(self, emb: np.ndarray, group: np.ndarray) -> Tuple[np.ndarray, str]:
        """-> (the merges of height <= threshold as dendrogram rows, the backend that made them)"""
        use_hip = self.backend == "hip" or (self.backend == "auto" and len(emb) >= HIP_LINK_MIN and clustering._hip_ready())
        if use_hip and self.backend == "auto" and clustering._has_duplicate_rows(emb):
            use_hip = False               # exact ties
        if use_hip:
            from . import ops
            from ._lib import DznError
            try:
                self.device_calls += 1
                Z, m = ops.link_speakers(emb, group, self.threshold, device=_device_index(self.device))
                return Z[:m], "hip"
            except (DznError, MemoryError):
                if self.backend == "hip":
                    raise
        Z, m = link_scipy(emb, group, self.threshold)
        return Z, "scipy"

    def link(self) -> SpeakerLinks:
        keys = [(rec, lab) for rec, labs in zip(self._recordings, self._labels) for lab in labs]
        all_rows = np.concatenate(self._rows) if self._rows else np.zeros((0, self.dim), dtype=np.float32)
        group = np.concatenate([np.full(len(r), g, dtype=np.int32) for g, r in enumerate(self._rows)]) if self._rows else \
            np.zeros((0,), dtype=np.int32)
        good = _usable(all_rows) if len(all_rows) else np.zeros((0,), dtype=bool)
        idx = np.flatnonzero(good)
        n = len(idx)
        cluster = np.full(len(all_rows), -1, dtype=np.int64)      # per row: a cluster key (usable rows), -1 = on its own
        height = np.zeros(0)
        backend = "trivial"
        if n >= 2:
            emb = np.ascontiguousarray(all_rows[idx])
            merges, backend = self._merges(emb, group[idx])
            if backend == "scipy":
                from scipy.cluster.hierarchy import fcluster
                flat = fcluster(merges, self.threshold, "distance")
                root, height = _union_find(n, merges[merges[:, 2] <= self.threshold])
                assert len(set(zip(flat.tolist(), root.tolist()))) == len(set(root.tolist()))      # the same partition
            else:
                root, height = _union_find(n, merges)
            cluster[idx] = root
        elif n == 1:
            cluster[idx] = 0
            height = np.zeros(1)
        ids, number, diameter = [], {}, {}
        for r in range(len(all_rows)):
            c = int(cluster[r])
            if c < 0 or c not in number:
                i = len(diameter)
                diameter[i] = float(height[c]) if c >= 0 else 0.0
                if c >= 0:
                    number[c] = i
            else:
                i = number[c]
            ids.append(i)
        unusable = [k for k, ok in zip(keys, good) if not ok]
        return SpeakerLinks(keys, ids, diameter, unusable, self.threshold, backend)
