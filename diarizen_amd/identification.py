"""Speaker identification: which of the enrolled people is speaker 2?

No reference counterpart: the reference (and every pipeline here) ends at anonymous integer labels.  A voiceprint is a cluster
centroid of the embeddings the engine already produces (overlap-excluded masks, 8-16 s windows) — `DiariZenPipeline.voiceprint`
for enrolment, `__call__(return_embeddings=True)` / `LiveDiarization.centroids` at test time — so enrolment and test live in the
same space and no further model path is involved.

  SpeakerGallery          names <-> rows of a device-resident gallery (csrc/gallery.hip, ops.GalleryState).  The bookkeeping is
                          host-only; the device state is created and synchronised lazily at the first `search`.
  assign_identities       the one-to-one rule inside one recording / session (pure host function)
  SpeakerIdentification   pipeline + gallery + threshold -> (Annotation with names, [Identity]); `identify_live` for live
                          sessions, one search for all of them

The threshold is required everywhere and has no default: a cosine operating point can only come from real checkpoints and
real speakers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .core import Annotation


def _device_index(device) -> int:
    if device is None:
        return -1
    if isinstance(device, (int, np.integer)):
        return int(device)
    idx = getattr(device, "index", None)
    return 0 if idx is None else int(idx)


def _check_name(name) -> str:
    if not isinstance(name, str) or not name or any(ch.isspace() for ch in name):
        raise ValueError(f"a gallery name is a non-empty string without whitespace (it ends up in RTTM), not {name!r}")
    return name


def _usable(rows: np.ndarray) -> np.ndarray:
    """bool [n]: rows that are finite and not all zero (what the library accepts)"""
    return np.isfinite(rows).all(axis=1) & (rows != 0).any(axis=1)


class SpeakerGallery:
    def __init__(self, dim: int = 256, device=None, capacity: int = 1024):
        """dim: the embedding dimension (a multiple of 16, 16 .. 512); device: a torch.device, an ordinal or None (the current
        device); capacity: rows allocated on the device at first, doubled whenever the names outgrow it."""
        if dim < 16 or dim > 512 or dim % 16:
            raise ValueError(f"dim is a multiple of 16 in 16 .. 512, not {dim!r}")
        if capacity < 1:
            raise ValueError(f"capacity must be at least 1, not {capacity!r}")
        self.dim, self.device, self.capacity = int(dim), device, int(capacity)
        self._raw = np.zeros((self.capacity, self.dim), dtype=np.float32)    # the voiceprints as given (the device normalises)
        self._slot: Dict[str, int] = {}
        self._name: List[Optional[str]] = []                                 # per slot ever used: its name or None (free)
        self._free: List[int] = []
        self._dirty: set = set()
        self._state = None
        self.searches = 0                                                    # library search calls made

    # ------------------------------------------------------------------ bookkeeping (host only)
    def __len__(self) -> int:
        return len(self._slot)

    def __contains__(self, name) -> bool:
        return name in self._slot

    @property
    def names(self) -> List[str]:
        """the enrolled names in slot order"""
        return [n for n in self._name if n is not None]

    def slot_of(self, name: str) -> int:
        return self._slot[name]

    def voiceprint(self, name: str) -> np.ndarray:
        """the voiceprint as enrolled (a copy)"""
        return self._raw[self._slot[name]].copy()

    def enroll(self, name: str, voiceprint) -> int:
        """one row per name; enrolling a name again replaces its row.  Returns the slot."""
        _check_name(name)
        v = np.asarray(voiceprint, dtype=np.float32).reshape(-1)
        if v.shape != (self.dim,):
            raise ValueError(f"a voiceprint has {self.dim} values, not {v.shape}")
        if not _usable(v[None])[0]:
            raise ValueError(f"the voiceprint of {name!r} is all zero or not finite")
        slot = self._slot.get(name)
        if slot is None:
            if self._free:
                self._free.sort()
                slot = self._free.pop(0)
            else:
                slot = len(self._name)
                self._name.append(None)
                if slot >= self.capacity:
                    self._grow()
            self._slot[name] = slot
            self._name[slot] = name
        self._raw[slot] = v
        self._dirty.add(slot)
        return slot

    def remove(self, name: str) -> None:
        slot = self._slot.pop(name)
        self._name[slot] = None
        self._raw[slot] = 0.0
        self._free.append(slot)
        self._dirty.add(slot)

    def _grow(self) -> None:
        self.capacity *= 2
        raw = np.zeros((self.capacity, self.dim), dtype=np.float32)
        raw[:len(self._raw)] = self._raw
        self._raw = raw          # the device handle is replaced at the next search (_sync)

    def save(self, path) -> None:
        """an .npz with the names and the raw float32 voiceprints, in slot order"""
        names = self.names
        rows = self._raw[[self._slot[n] for n in names]] if names else np.zeros((0, self.dim), dtype=np.float32)
        with open(path, "wb") as f:
            np.savez(f, names=np.array(names, dtype=np.str_), voiceprints=np.ascontiguousarray(rows, dtype=np.float32),
                     dim=np.int64(self.dim))

    @classmethod
    def load(cls, path, device=None) -> "SpeakerGallery":
        with np.load(path, allow_pickle=False) as z:
            names, rows, dim = [str(n) for n in z["names"]], z["voiceprints"], int(z["dim"])
        if rows.dtype != np.float32 or rows.shape != (len(names), dim):
            raise ValueError(f"{path}: voiceprints are float32 [{len(names)}, {dim}], not {rows.dtype} {rows.shape}")
        g = cls(dim=dim, device=device, capacity=max(1024, len(names)))
        for n, r in zip(names, rows):
            g.enroll(n, r)
        return g

    # ------------------------------------------------------------------ device
    def _runs(self, slots: Sequence[int]):
        """ascending slots -> (first, count) of every contiguous run"""
        run = []
        for s in sorted(slots):
            if run and s == run[-1] + 1:
                run.append(s)
            else:
                if run:
                    yield run[0], len(run)
                run = [s]
        if run:
            yield run[0], len(run)

    def _sync(self):
        from . import ops
        if self._state is not None and self._state.capacity < self.capacity:
            self._state.close()
            self._state = None
        if self._state is None:
            self._state = ops.GalleryState(self.dim, self.capacity, _device_index(self.device))
            live = sorted(self._slot.values())
            self._dirty.clear()
        else:
            live = [s for s in self._dirty if self._name[s] is not None]
        for s0, n in self._runs(live):
            self._state.put(s0, self._raw[s0:s0 + n])
        for s0, n in self._runs([s for s in self._dirty if self._name[s] is None]):
            self._state.drop(s0, n)
        self._dirty.clear()
        return self._state

    def search_slots(self, queries, top_n: int) -> Tuple[np.ndarray, np.ndarray]:
        """queries [Q, dim] -> (scores f32 [Q, top_n], slots i64 [Q, top_n]): per query the best enrolled rows by (cosine
        descending, slot ascending), slot -1 / score -inf beyond the number of enrolled names.  A query that is all zero or
        not finite is answered here with an all -1 row and is not sent to the library."""
        q = np.asarray(queries, dtype=np.float32).reshape(-1, self.dim)
        top_n = int(top_n)
        if top_n < 1:
            raise ValueError(f"top_n must be at least 1, not {top_n}")
        scores = np.full((len(q), top_n), -np.inf, dtype=np.float32)
        slots = np.full((len(q), top_n), -1, dtype=np.int64)
        good = _usable(q)
        if good.any():
            state = self._sync()
            s, i = state.search(q[good], top_n)
            self.searches += 1
            scores[good], slots[good] = s, i
        return scores, slots

    def search(self, queries, top_n: int):
        """-> (scores f32 [Q, top_n], names [Q][top_n]) with None where there is no further enrolled name"""
        scores, slots = self.search_slots(queries, top_n)
        return scores, [[self._name[i] if i >= 0 else None for i in row] for row in slots]

    def close(self) -> None:
        if self._state is not None:
            self._state.close()
            self._state = None


def assign_identities(scores, slots, threshold: float) -> list:
    """scores [K, n], slots [K, n] (slot -1 = no candidate): the candidate lists of the K labels of ONE recording or session ->
    list of K entries, the slot matched to label k or None.

    One-to-one: two labels never get the same slot.  Among all such partial matchings of labels to listed candidates with
    score >= threshold it maximises the sum of (score - threshold); any label may stay unmatched at gain 0.  Solved with
    scipy.optimize.linear_sum_assignment on the union of the candidates.

    Callers search with top_n = min(K, len(gallery)).  With n >= K the restriction to per-label top-n lists loses nothing: take
    an optimal matching on the dense scores in which some label k holds a slot outside its top n.  At most K - 1 of the n >= K
    slots listed for k are held by other labels, so one of them is free, and it scores at least as much for k as the slot
    held; exchanging keeps the matching one-to-one and does not lower the objective.  Repeating this for every such label
    gives an optimal matching inside the lists."""
    from scipy.optimize import linear_sum_assignment
    scores = np.asarray(scores, dtype=np.float64)
    slots = np.asarray(slots, dtype=np.int64)
    K = scores.shape[0]
    out: list = [None] * K
    ok = (slots >= 0) & (scores >= threshold)          # (NaN and -inf compare False)
    cand = np.unique(slots[ok])
    if K == 0 or len(cand) == 0:
        return out
    col = {int(s): j for j, s in enumerate(cand)}
    gain = np.zeros((K, len(cand)), dtype=np.float64)
    allowed = np.zeros((K, len(cand)), dtype=bool)
    for k in range(K):
        for s, v in zip(slots[k][ok[k]], scores[k][ok[k]]):
            j = col[int(s)]
            if not allowed[k, j] or v - threshold > gain[k, j]:
                gain[k, j] = v - threshold
                allowed[k, j] = True
    for k, j in zip(*linear_sum_assignment(gain, maximize=True)):
        if allowed[k, j]:
            out[int(k)] = int(cand[j])
    return out


@dataclass(frozen=True)
class Identity:
    """label: the diarization label; name: the enrolled name matched to it, or None; score: the cosine to `name` (None when
    unmatched); runner_up / runner_up_score: the best-scoring enrolled name other than `name` and its cosine (None without one)"""
    label: object
    name: Optional[str]
    score: Optional[float]
    runner_up: Optional[str]
    runner_up_score: Optional[float]


def relabel(annotation: Annotation, names: Dict) -> Annotation:
    """the annotation with every label found in `names` replaced by its name; other labels are kept"""
    out = Annotation(uri=annotation.uri, modality=getattr(annotation, "modality", None))
    for segment, track, label in annotation.itertracks(yield_label=True):
        out[segment, track] = names.get(label, label)
    return out


class SpeakerIdentification:
    MAX_TOP_N = 32          # the library's max_top_n

    def __init__(self, pipeline, gallery: SpeakerGallery, *, threshold: float):
        """threshold: the cosine a label's centroid must reach against an enrolled voiceprint to take its name.  Required, no
        default: an operating point can only be calibrated on real checkpoints and real speakers."""
        self.pipeline, self.gallery, self.threshold = pipeline, gallery, float(threshold)

    def _top_n(self, K: int) -> int:
        return max(1, min(K, len(self.gallery), self.MAX_TOP_N))

    def _identities(self, labels: Sequence, scores: np.ndarray, slots: np.ndarray) -> List[Identity]:
        name_of = self.gallery._name
        matched = assign_identities(scores, slots, self.threshold)
        out = []
        for k, label in enumerate(labels):
            m = matched[k]
            score = None
            ru = ru_s = None
            for s, i in zip(scores[k], slots[k]):          # (score descending)
                if i < 0:
                    continue
                if m is not None and int(i) == m:
                    score = float(s)
                elif ru is None:
                    ru, ru_s = name_of[int(i)], float(s)
            out.append(Identity(label, name_of[m] if m is not None else None, score, ru, ru_s))
        return out

    def identify(self, centroids, labels: Optional[Sequence] = None) -> List[Identity]:
        """centroids [K, dim] of ONE recording or session (row k = label k unless `labels` names them) -> K identities"""
        c = np.asarray(centroids, dtype=np.float32).reshape(-1, self.gallery.dim)
        labels = list(range(len(c))) if labels is None else list(labels)
        if len(c) == 0:
            return []
        scores, slots = self.gallery.search_slots(c, self._top_n(len(c)))
        return self._identities(labels, scores, slots)

    def __call__(self, wav, sess_name: Optional[str] = None):
        """-> (Annotation, [Identity]): the pipeline's annotation with matched labels replaced by names (unmatched labels are
        kept; the pipeline's own RTTM file is unchanged) and one Identity per cluster, label k = row k of the embeddings"""
        annotation, embeddings = self.pipeline(wav, sess_name=sess_name, return_embeddings=True)
        if annotation is None:                             # a rank other than 0 of a sharded run
            return None, []
        ids = self.identify(embeddings)
        return relabel(annotation, {i.label: i.name for i in ids if i.name is not None}), ids

    def identify_live(self, sessions: Iterable) -> Dict[str, List[Identity]]:
        """live.LiveDiarization sessions (e.g. hub.sessions.values()) -> {session name: [Identity per label opened so far]}.
        ONE search for the centroids of all sessions together, then one assignment per session.  Live labels and annotations
        are not renamed — labels never change; a name may, as a centroid matures."""
        sessions = list(sessions)
        cents = [np.asarray(s.centroids, dtype=np.float32).reshape(-1, self.gallery.dim) for s in sessions]
        out: Dict[str, List[Identity]] = {s.name: [] for s in sessions}
        total = sum(len(c) for c in cents)
        if total == 0:
            return out
        scores, slots = self.gallery.search_slots(np.concatenate(cents), self._top_n(max(len(c) for c in cents)))
        at = 0
        for s, c in zip(sessions, cents):
            out[s.name] = self._identities(list(range(len(c))), scores[at:at + len(c)], slots[at:at + len(c)])
            at += len(c)
        return out
