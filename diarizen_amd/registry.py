"""A speaker registry: link new recordings into a growing corpus, one recording at a time.

No reference counterpart.  `linking.SpeakerLinker` answers "is Monday's speaker 2 Tuesday's speaker 0?" for a corpus that is
complete before `link()` runs: the whole n x n matrix and the whole complete-linkage loop per call, and identity numbers that
follow the clustering.  A registry is the persistent counterpart: a set of identities that a finished recording is matched
against in one sweep, whose numbers never change once given.

State: N stored voiceprints (float32 [N, dim], as given), each with an identity number and the recording it came from; no
identity holds two rows of one recording.  Adding recording R with usable voiceprints q_0 .. q_{K-1}:

    D[k, i] = max over the stored rows r of identity i of cosdist(q_k, E_r)      (float64 cosine distance, dzn_cdist_cosine's)

and complete linkage is CONTINUED over the I + K nodes "identity i" and "new row k": identity-identity and new-new distances
are BIG (two existing identities never merge afterwards; two labels of one recording are different people), identity-new is
D[k, i], cut at the threshold.  As scipy: that (I + K)^2 matrix, linkage(condensed, "complete"), fcluster(Z, threshold,
"distance"); row k joins identity i iff they share a flat cluster.  Because every merge strikes a whole row and column (the
max with a BIG entry is BIG), this is the greedy rule `greedy_assign` runs: take the smallest remaining D[k, i]; at or below
the threshold assign k -> i and strike row k and column i; otherwise stop.  Exact ties: the lowest (k, i) wins.

Unassigned rows found new identities in label order (an unusable row — all zero or not finite — always does, and is never
stored).  On assignment diameter[i] = max(diameter[i], D[k, i]): any two voiceprints of an identity are at most
diameter[i] <= threshold apart, the guarantee `SpeakerLinks.diameter` states.

Two limits of any incremental rule: the result depends on arrival order, and two existing identities are never merged
afterwards (`batch_links()` runs the batch linker over the stored rows to audit the drift).

backend "numpy" is the definition in float64; "hip" is csrc/registry.hip (dzn_registry_match: one sweep over the stored rows
per group of up to 32 queries, only the (k, i, d) triples <= threshold come back).  The host copy of rows and identities is
the authoritative one; the device copy is a cache that catches up before a device match and that `load` rebuilds."""
from __future__ import annotations

import json
import warnings
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np

from . import clustering
from .identification import _device_index, _usable
from .linking import SpeakerLinker, SpeakerLinks

# "auto" takes the device from this many stored voiceprints up.  Measured on one idle MI355X (scripts/registry_timing.py ->
# profiles/registry_timing.json, one add of K = 8 at dim 256): the device add (append + index upload + match) and the numpy
# backend meet at N = 256 (0.20 against 0.17 ms) and the device is 2.8x ahead at 1000 (0.20 against 0.57 ms), 128x at 100 000; 1024
# leaves that factor for a device that is busy with a pipeline's windows.
REGISTRY_HIP_MIN = 1024

_CHUNK = 65536      # stored rows converted to float64 at a time by the numpy backend


def cosine_table(queries: np.ndarray, rows: np.ndarray, ident: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """the definition in float64 -> (columns int [C]: the identity numbers that hold a row, ascending; D float64 [K, C]: per
    query the max over the identity's rows of 1 - clip(dot / (|q||e|)))"""
    q = np.asarray(queries).astype(np.float64)
    nq = np.sqrt((q * q).sum(axis=1))
    cols, inv = np.unique(np.asarray(ident), return_inverse=True)
    D = np.full((len(q), len(cols)), -np.inf)
    for r0 in range(0, len(rows), _CHUNK):
        e = np.asarray(rows[r0:r0 + _CHUNK]).astype(np.float64)
        ne = np.sqrt((e * e).sum(axis=1))
        cos = np.clip((q @ e.T) / (nq[:, None] * ne[None, :]), -1.0, 1.0)
        dist = 1.0 - cos
        c = inv[r0:r0 + _CHUNK]
        order = np.argsort(c, kind="stable")
        starts = np.flatnonzero(np.diff(c[order], prepend=-1))
        part = np.maximum.reduceat(dist[:, order], starts, axis=1)
        here = c[order][starts]
        D[:, here] = np.maximum(D[:, here], part)
    return cols, D


def greedy_assign(k: np.ndarray, i: np.ndarray, d: np.ndarray, threshold: float) -> Dict[int, Tuple[int, float]]:
    """(k, i, d) entries of the table (any superset of those <= threshold) -> {k: (i, d)}: the smallest remaining entry is
    assigned and strikes its row and column until the smallest is above the threshold; ties go to the lowest (k, i)"""
    out: Dict[int, Tuple[int, float]] = {}
    taken = set()
    for j in np.lexsort((i, k, d)):
        if d[j] > threshold:
            break
        kk, ii = int(k[j]), int(i[j])
        if kk in out or ii in taken:
            continue
        out[kk] = (ii, float(d[j]))
        taken.add(ii)
    return out


class SpeakerRegistry:
    def __init__(self, threshold: float, dim: int = 256, capacity: int = 1 << 16, device=None, backend: str = "auto"):
        """threshold: the cosine DISTANCE up to which a new voiceprint joins an identity, in (0, 2].  Required, no default:
        nothing here can calibrate one (seeded weights only).  capacity: the stored voiceprints the registry (and
        its device allocation, capacity * dim * 4 bytes) can hold; an `add` that does not fit raises MemoryError and changes
        nothing.  device: a torch.device, an ordinal or None (the current device).  backend: "numpy", "hip" (raises when the
        device path fails; dim must be a multiple of 4, at most 1024) or "auto": the device from REGISTRY_HIP_MIN stored
        voiceprints up when a device and the library are present, numpy otherwise; when a device call fails it warns once,
        records the reason in `device_error` and stays with numpy."""
        threshold = float(threshold)
        if not (0.0 < threshold <= 2.0):
            raise ValueError(f"threshold is a cosine distance in (0, 2], not {threshold!r}")
        if backend not in ("auto", "numpy", "hip"):
            raise ValueError(f"unknown registry backend {backend!r}")
        if int(dim) < 1:
            raise ValueError(f"dim must be at least 1, not {dim!r}")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be at least 1, not {capacity!r}")
        self.threshold, self.dim, self.capacity, self.device, self.backend = threshold, int(dim), int(capacity), device, backend
        self._rows = np.zeros((min(self.capacity, 1024), self.dim), dtype=np.float32)      # grows by doubling up to capacity
        self._ident = np.zeros(len(self._rows), dtype=np.int32)
        self._n = 0
        self._recordings: List[Hashable] = []
        self._names = set()                       # of the recordings
        self._labels: List[list] = []
        self._ids: List[List[int]] = []           # per recording, per label: its identity
        self._usable: List[List[bool]] = []       # per recording, per label: stored or not
        self.diameter: Dict[int, float] = {}
        self._state = None                        # ops.Registry: the device cache
        self._device_rows = 0                     # rows of the host copy the device holds
        self._used_hip = False
        self.device_error: Optional[str] = None   # "auto": why the device was given up (it is not tried again)
        self.device_calls = 0                     # library match calls made

    # ------------------------------------------------------------------ views
    def __len__(self) -> int:
        """the stored (usable) voiceprints"""
        return self._n

    def __contains__(self, recording) -> bool:
        """whether a recording of that name was added"""
        return recording in self._names

    @property
    def num_identities(self) -> int:
        return len(self.diameter)

    @property
    def identity(self) -> Dict[Tuple[Hashable, Hashable], int]:
        return {(rec, lab): i for rec, labs, ids in zip(self._recordings, self._labels, self._ids) for lab, i in zip(labs, ids)}

    @property
    def unusable(self) -> List[Tuple[Hashable, Hashable]]:
        return [(rec, lab) for rec, labs, oks in zip(self._recordings, self._labels, self._usable)
                for lab, ok in zip(labs, oks) if not ok]

    @property
    def rows(self) -> np.ndarray:
        """the stored voiceprints float32 [N, dim] (a read-only view)"""
        v = self._rows[:self._n]
        v.setflags(write=False)
        return v

    @property
    def row_identity(self) -> np.ndarray:
        """the identity of every stored row, int32 [N]"""
        return self._ident[:self._n].copy()

    def links(self) -> SpeakerLinks:
        """the registry as the batch linker's result class: identity, members, diameter, names / relabel"""
        keys = [(rec, lab) for rec, labs in zip(self._recordings, self._labels) for lab in labs]
        ids = [i for rec_ids in self._ids for i in rec_ids]
        return SpeakerLinks(keys, ids, self.diameter, self.unusable, self.threshold, "hip" if self._used_hip else "numpy")

    # ------------------------------------------------------------------ the device cache
    def _device(self):
        from . import ops
        if self._state is None:
            self._state = ops.Registry(self.dim, self.capacity, device=_device_index(self.device))
            self._device_rows = 0
        if self._device_rows < self._n:
            self._state.append(self._rows[self._device_rows:self._n], self._ident[self._device_rows:self._n])
            self._device_rows = self._n
        return self._state

    def _matches(self, q: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, bool]:
        """-> (k, i, d, on the device): at least the entries <= threshold of the table"""
        empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
        if len(q) == 0 or self._n == 0:
            return empty + (False,)
        use_hip = self.backend == "hip" or (self.backend == "auto" and self.device_error is None and
                                            self._n >= REGISTRY_HIP_MIN and clustering._hip_ready())
        if use_hip:
            from ._lib import DznError
            try:
                state = self._device()
                self.device_calls += 1
                return state.match(q, self.threshold) + (True,)
            except (DznError, MemoryError) as e:
                if self.backend == "hip":
                    raise
                self.close()                      # "auto": the host takes over for good, one warning says so
                self.device_error = f"{type(e).__name__}: {e}"
                warnings.warn(f"SpeakerRegistry: the device path failed ({self.device_error}); continuing with the numpy backend")
        cols, D = cosine_table(q, self._rows[:self._n], self._ident[:self._n])
        k, c = np.nonzero(D <= self.threshold)
        return k.astype(np.int32), cols[c].astype(np.int32), D[k, c], False

    # ------------------------------------------------------------------ add
    def _grow(self, need: int) -> None:
        if need > len(self._rows):
            size = min(self.capacity, max(need, 2 * len(self._rows)))
            rows, ident = np.zeros((size, self.dim), dtype=np.float32), np.zeros(size, dtype=np.int32)
            rows[:self._n], ident[:self._n] = self._rows[:self._n], self._ident[:self._n]
            self._rows, self._ident = rows, ident

    def add(self, recording, voiceprints, labels: Optional[Sequence] = None) -> Dict:
        """the K voiceprints of one finished recording: float32 [K, dim] (row k = label k unless `labels` names them), or a
        live.LiveDiarization (its `centroids`) -> {label: identity}.  K = 0 is allowed; a recording name can be added once.
        A refused add (duplicate name or labels, no room left, a failing device with backend "hip") changes nothing."""
        if recording in self._names:
            raise ValueError(f"recording {recording!r} was added before")
        rows = getattr(voiceprints, "centroids", voiceprints)
        rows = np.array(rows, dtype=np.float32, copy=True).reshape(-1, self.dim) if np.size(rows) else \
            np.zeros((0, self.dim), dtype=np.float32)
        labels = list(range(len(rows))) if labels is None else list(labels)
        if len(labels) != len(rows) or len(set(labels)) != len(labels):
            raise ValueError(f"{recording!r}: one distinct label per voiceprint ({len(rows)} rows, labels {labels!r})")
        good = _usable(rows) if len(rows) else np.zeros((0,), dtype=bool)
        idx = np.flatnonzero(good)
        if self._n + len(idx) > self.capacity:
            raise MemoryError(f"{recording!r}: {len(idx)} voiceprints do not fit ({self._n} of {self.capacity} stored)")
        q = np.ascontiguousarray(rows[idx])
        k, i, d, on_device = self._matches(q)
        assigned = greedy_assign(k, i, d, self.threshold)
        # ---- commit
        ids, nxt = [], len(self.diameter)
        diameter = dict(self.diameter)
        pos = {int(r): j for j, r in enumerate(idx)}
        for r in range(len(rows)):
            hit = assigned.get(pos[r]) if r in pos else None
            if hit is None:
                ids.append(nxt)
                diameter[nxt] = 0.0
                nxt += 1
            else:
                ids.append(hit[0])
                diameter[hit[0]] = max(diameter[hit[0]], hit[1])
        self._grow(self._n + len(idx))
        self._rows[self._n:self._n + len(idx)] = q
        self._ident[self._n:self._n + len(idx)] = [ids[int(r)] for r in idx]
        self._n += len(idx)
        self.diameter = diameter
        self._recordings.append(recording)
        self._names.add(recording)
        self._labels.append(labels)
        self._ids.append(ids)
        self._usable.append([bool(g) for g in good])
        self._used_hip |= on_device
        return dict(zip(labels, ids))

    # ------------------------------------------------------------------ the batch linker: seed from it, audit against it
    @classmethod
    def from_links(cls, linker: SpeakerLinker, links: SpeakerLinks, capacity: int = 1 << 16, device=None,
                   backend: str = "auto") -> "SpeakerRegistry":
        """a registry seeded from a finished batch run: the linker's recordings and voiceprints under the identities, diameters
        and threshold of its `link()` result"""
        reg = cls(links.threshold, dim=linker.dim, capacity=capacity, device=device, backend=backend)
        total = sum(int(_usable(r).sum()) if len(r) else 0 for r in linker._rows)
        if total > reg.capacity:
            raise MemoryError(f"{total} voiceprints do not fit a capacity of {reg.capacity}")
        reg._grow(total)
        for rec, rows, labels in zip(linker._recordings, linker._rows, linker._labels):
            good = _usable(rows) if len(rows) else np.zeros((0,), dtype=bool)
            ids = [int(links.identity[(rec, lab)]) for lab in labels]
            n = int(good.sum())
            reg._rows[reg._n:reg._n + n] = rows[good]
            reg._ident[reg._n:reg._n + n] = [i for i, g in zip(ids, good) if g]
            reg._n += n
            reg._recordings.append(rec)
            reg._names.add(rec)
            reg._labels.append(list(labels))
            reg._ids.append(ids)
            reg._usable.append([bool(g) for g in good])
        reg.diameter = {int(i): float(v) for i, v in links.diameter.items()}
        return reg

    def batch_links(self, backend: Optional[str] = None) -> SpeakerLinks:
        """the batch SpeakerLinker over everything stored, in `add` order (an unusable voiceprint stands in as a zero row): what
        one complete-linkage run over the same corpus gives, to audit the arrival-order drift"""
        if backend is None:
            backend = "scipy" if self.backend == "numpy" else self.backend
        linker = SpeakerLinker(self.threshold, dim=self.dim, device=self.device, backend=backend)
        at = 0
        for rec, labels, oks in zip(self._recordings, self._labels, self._usable):
            rows = np.zeros((len(labels), self.dim), dtype=np.float32)
            n = sum(oks)
            rows[np.array(oks, dtype=bool)] = self._rows[at:at + n]
            at += n
            linker.add(rec, rows, labels)
        return linker.link()

    # ------------------------------------------------------------------ persistence
    def save(self, path) -> None:
        """one .npz (loadable with allow_pickle=False): rows, identities, threshold, diameters, and the recording names, labels
        and per-label identities as JSON text — names and labels must survive JSON (strings, integers)"""
        meta = {"recordings": self._recordings, "labels": self._labels, "ids": self._ids, "usable": self._usable,
                "dim": self.dim, "capacity": self.capacity, "backend": self.backend}
        text = json.dumps(meta)
        back = json.loads(text)
        if back["recordings"] != self._recordings or back["labels"] != self._labels:
            raise ValueError("recording names and labels must be JSON values (strings, integers) to be saved")
        diam = np.array([self.diameter[i] for i in range(len(self.diameter))], dtype=np.float64)
        with open(path, "wb") as f:
            np.savez(f, rows=self._rows[:self._n], ident=self._ident[:self._n], threshold=np.float64(self.threshold),
                     diameter=diam, meta=np.array(text))

    @classmethod
    def load(cls, path, device=None, backend: Optional[str] = None) -> "SpeakerRegistry":
        """the registry `save` wrote; the device copy is rebuilt by the first device match"""
        with np.load(path, allow_pickle=False) as z:
            rows, ident, threshold, diam, text = z["rows"], z["ident"], float(z["threshold"]), z["diameter"], str(z["meta"])
        meta = json.loads(text)
        reg = cls(threshold, dim=meta["dim"], capacity=meta["capacity"], device=device, backend=backend or meta["backend"])
        reg._grow(len(rows))
        reg._rows[:len(rows)], reg._ident[:len(rows)], reg._n = rows, ident, len(rows)
        reg._recordings, reg._labels = list(meta["recordings"]), [list(x) for x in meta["labels"]]
        reg._names = set(reg._recordings)
        reg._ids, reg._usable = [list(x) for x in meta["ids"]], [list(x) for x in meta["usable"]]
        reg.diameter = {i: float(v) for i, v in enumerate(diam)}
        return reg

    def close(self) -> None:
        """free the device copy (the host copy stays; a later device match uploads it again)"""
        if self._state is not None:
            self._state.close()
            self._state = None
            self._device_rows = 0
