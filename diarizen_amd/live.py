"""Live speaker diarization: who is speaking now, under a label that does not change.

    live = pipeline.open_live(sess_name="meeting")
    for chunk in microphone:                               # float32 arrays at the pipeline's rate
        ann = live.feed(chunk)                             # None until the first window is complete
        ...                                                # final before live.committed_seconds, provisional after
    ann = live.finish()                                    # or finish(recluster=True): the offline result under the live labels

    for seconds, committed_seconds, ann in pipeline.stream_live(chunks, sess_name="meeting"): ...

The session is a streaming.CommittedStream, as detection.DetectionStream is: every window runs ONCE through the pipeline's own
runner (median filter, overlap-excluded embedding masks: the offline per-window bits), its decisions join one device buffer u8
[cmax, L, S], and per feed one range kernel computes only the frames the new windows touch.  What detection does not need and
diarization does — a global label for every local speaker — comes from online.OnlineSpeakers on the host, window by window and
never revised: only the decisions and embeddings of the NEW windows go to the host, only the new rows of the device hard
buffer int8 [cmax, S] go back, and dzn_diarize_range (csrc/post.hip) does count -> reconstruct -> top-count for
[frontier, frames covered).

A frame's count, activations and selection depend only on the windows that cover it and on their labels, and a window's
labels are fixed when it is assigned.  With windows 0 .. C - 1 done, every frame before the start frame of window C (the
FRONTIER, postprocess.committed_frames) is therefore final, label included: `committed_diarization` / `committed_count` only
grow.  The frames from the frontier to the end of window C - 1 are the provisional tail, which the next window revises.
K, the number of label columns, is fixed for the session (min(max_speakers, 32)); the count is capped at the same value.
As in the reference's selection a frame whose count exceeds the number of labels with an activation takes zero activations
too, in ascending k, so a column k >= num_speakers can be active.
Ties at the selection boundary go to the smaller label (dzn_diarize_range) — the offline path reproduces numpy's own tie
order, so on tied frames the two may pick different speakers; the live rule is what makes a range call equal the whole.

min_cluster_size is not applied online, so a spurious small speaker is possible; finish(recluster=True) runs the ordinary host
stage over all windows and returns ITS annotation under the live labels (offline clusters are matched to live speakers by the
number of frames in which both are active).

Scores (`open_live(scores=True)`): the per-speaker activity scores of `pipeline(wav, return_scores=True)`, live.  The session
then also keeps the soft multilabel scores of its windows on the device, f32 [cmax, L, S] beside the decisions, and its one
range call per feed is dzn_diarize_range_scores: the same launch, whose lane (t, k) also walks the soft rows of its covering
windows (csrc/post.hip).  A frame's score depends on the windows that cover it and on their labels only, so
`committed_scores` [F, K] is as final as `committed_diarization` and has its rows; column k is label k.  The soft scores never
travel to the host; only the [n, K] rows of a range call do, with the decisions'.  Without scores=True nothing is allocated,
the classifier writes no soft output and the range call is dzn_diarize_range."""
from __future__ import annotations

from typing import Iterable, Iterator, Optional, Tuple

import numpy as np
import torch

from .core import Annotation, SlidingWindowFeature
from .online import OnlineSpeakers
from .postprocess import (_frame_grid, activity_regions, aggregation_windows, crop_end, diarize_range_launch,
                          diarize_range_scores_launch)
from .streaming import CommittedStream, stream_committed


def check_scores(scores) -> bool:
    """the `scores=` keyword of a live session: True or False, nothing that merely converts to one"""
    if not isinstance(scores, (bool, np.bool_)):
        raise ValueError(f"scores is True or False, not {scores!r}")
    return bool(scores)


def place_columns(data: np.ndarray, label_map: dict, K: int) -> np.ndarray:
    """offline scores f32 [T, Ko] -> f32 [T, max(K, largest label + 1)] with offline column i at column label_map[i]; a column
    nobody maps to is zeros"""
    width = max([int(K)] + [int(v) + 1 for v in label_map.values()])
    out = np.zeros((len(data), width), dtype=np.float32)
    for i in range(data.shape[1]):
        out[:, int(label_map[i])] = data[:, i]
    return out


class LiveDiarization(CommittedStream):
    def __init__(self, pipeline, sess_name: Optional[str] = None, delta_new: Optional[float] = None,
                 max_speakers: Optional[int] = None, max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0,
                 slots: int = 4, feed_format=None, hub=None, scores: bool = False):
        """delta_new: the distance beyond which a clean local speaker opens a new label (default: the pipeline's
        ahc_threshold); max_speakers: the cap on labels (default: the pipeline's, at most 32); max_seconds, slot_seconds,
        slots: the ingest ring (streaming.WaveIngest); feed_format: an audio.FeedFormat when the feeds are the source's own
        bytes; hub: the hub.LiveHub whose tick() drives the session (pipeline.open_hub).
        scores=True: also `committed_scores` / `scores` / `final_scores`.  The session then holds the soft scores of its
        windows in a device buffer f32 [cmax, L, S] (cmax: the windows of max_seconds), cmax x L x S x 4 bytes: about 4.8 MB
        for a 600 s hub session, about 115 MB for a 4 h solo session; allocated only then."""
        self.SCORES = check_scores(scores)                              # (before anything is allocated)
        self.K = min(int(max_speakers or pipeline.max_speakers), 32)
        if self.K < 1:
            raise ValueError(f"max_speakers must be at least 1, not {max_speakers!r}")
        if delta_new is None:
            delta_new = pipeline.config["clustering"]["args"]["ahc_threshold"]
        rows = {"act": (np.uint8, (self.K,)), "cnt": (np.uint8, ())}
        if self.SCORES:
            rows["score"] = (np.float32, (self.K,))
        super().__init__(pipeline, sess_name, rows, max_seconds, slot_seconds, slots, feed_format, hub)
        S = self.seg.shape[2]
        self.hard = torch.full((len(self.seg), S), -2, device=self.device, dtype=torch.int8)       # the windows' global labels
        self.soft = self.d_ham = self.d_wu = None
        if self.SCORES:
            with torch.cuda.device(self.device):
                self.soft = torch.zeros(self.seg.shape, device=self.device, dtype=torch.float32)   # soft scores of every window so far
                self.d_ham, self.d_wu = (torch.from_numpy(w).to(self.device)
                                         for w in aggregation_windows(self.seg.shape[1], self.chunks.duration))
        self._final_scores = None
        self.speakers = OnlineSpeakers(delta_new, self.K, pipeline.engine.emb.embed_dim)
        self._seg_h, self._emb_h = [], []                               # per feed: the new windows' decisions / embeddings (host)
        self._hard_h = np.zeros((0, S), dtype=np.int8)
        self.label_map = None                                           # finish(recluster=True): offline cluster -> live label

    # ------------------------------------------------------------------ state
    @property
    def committed_diarization(self) -> np.ndarray:
        """u8 [F, K]: the speaker activity of the F committed frames, column k = label k (a copy)"""
        return self.rows.committed("act")

    @property
    def committed_count(self) -> np.ndarray:
        """u8 [F]: the (capped) instantaneous speaker count of the committed frames (a copy)"""
        return self.rows.committed("cnt")

    @property
    def committed_scores(self) -> Optional[np.ndarray]:
        """f32 [F, K]: the per-speaker activity scores of the F committed frames, column k = label k (a copy; the rows of
        committed_diarization), when the session was opened with scores=True"""
        return self.rows.committed("score") if self.SCORES else None

    @property
    def scores(self) -> Optional[SlidingWindowFeature]:
        """the scores of every frame computed so far (committed + provisional tail) on the session's frame grid, with scores=True"""
        return SlidingWindowFeature(self.rows.valid("score").copy(), self.grid) if self.SCORES else None

    @property
    def final_scores(self) -> Optional[np.ndarray]:
        """once the stream has ended (scores=True): f32 [T, K], the committed rows; after finish(recluster=True) the offline
        per-speaker scores of `pipeline(wav, return_scores=True)` (cropped at the end of the audio as there) with offline
        column i at column label_map[i], [T, max(K, largest label + 1)], columns nobody maps to zero"""
        if not self.SCORES or self.result is None:
            return None
        return self.committed_scores if self._final_scores is None else self._final_scores.copy()

    @property
    def num_speakers(self) -> int:
        """labels opened so far"""
        return self.speakers.num_speakers

    @property
    def centroids(self) -> np.ndarray:
        """float64 [num_speakers, dim]: the centroid of every label opened so far, row k = label k (a copy; what
        identification.SpeakerIdentification.identify_live scores against a gallery)"""
        return np.array(self.speakers.centroids, dtype=np.float64, copy=True)

    @property
    def hard_clusters(self) -> np.ndarray:
        """int8 [done, S]: the label of every local speaker of every window so far, -2 = none (a copy)"""
        return self._hard_h.copy()

    # ------------------------------------------------------------------ device / host work
    def _windows(self, res, lo: int, hi: int) -> None:
        """keep the new windows' decisions on the device, label them on the host and upload the new rows of the hard buffer"""
        super()._windows(res, lo, hi)
        if self.SCORES:
            self.soft[lo:hi] = res.scores                               # device to device: the soft scores stay there
        host = getattr(res, "host", None)                               # a hub's tick has fetched them for all sessions at once
        seg, emb = host if host is not None else (res.segmentations.cpu().numpy(), res.embeddings.cpu().numpy())     # the new windows only
        hard = np.stack([self.speakers.assign(seg[i], emb[i]) for i in range(hi - lo)])
        self.hard[lo:hi] = torch.from_numpy(hard).to(self.device)
        self._seg_h.append(seg)
        self._emb_h.append(emb)
        self._hard_h = np.concatenate([self._hard_h, hard])

    def _range(self, t0: int, t1: int, frontier: int) -> dict:
        if self.SCORES:                                                 # still ONE launch per feed
            cnt, act, _, sc = diarize_range_scores_launch(self.seg, self.hard, self.soft, self.done, self.d_start, self.d_ham,
                                                          self.d_wu, t0, t1, self.K, self.K)
            return {"act": act, "cnt": cnt, "score": sc}
        cnt, act, _ = diarize_range_launch(self.seg, self.hard, self.done, self.d_start, t0, t1, self.K, self.K)
        return {"act": act, "cnt": cnt}

    def _annotate(self) -> Annotation:
        return activity_regions(self.rows.valid("act").astype(bool), self.grid, uri=self.name)

    # ------------------------------------------------------------------ finish
    def finish(self, recluster: bool = False) -> Annotation:
        """end of stream: the zero-padded last window if the reference would run one, every frame committed (no crop at the
        end of the audio: the offline Annotation has none) -> the final Annotation, and its RTTM file when the pipeline has an
        rttm_out_dir and the session a name.
        recluster=True: the ordinary host stage (counting, AHC / VBx with min_cluster_size, reconstruction) over all windows;
        its clusters are matched to the live speakers (linear_sum_assignment, maximising the frames in which both are active;
        offline clusters left over get fresh labels from `num_speakers` upward) and ITS annotation is returned under the live
        labels; `label_map` keeps offline cluster -> live label.  The committed arrays stay the live ones.  With scores=True
        the host stage also aggregates the session's soft scores (still on the device) as `__call__(return_scores=True)` does:
        `final_scores`."""
        return super().finish(self._recluster if recluster else None)

    def _recluster(self) -> Annotation:
        from scipy.optimize import linear_sum_assignment
        got = {}
        kw = {}
        if self.SCORES:                                                 # the offline crop rule (pipeline.__call__)
            T = _frame_grid(self.done, self.seg.shape[1], self.chunks, self.frames)[2]
            if self._final_windows()[1]:
                T = crop_end(T, self.grid, self.n / self.sr)
            kw = dict(soft=self.soft[:self.done], num_frames=T)
        self.pipe.host_stage(np.concatenate(self._seg_h), np.concatenate(self._emb_h), self.name,
                             hook=lambda name, artifact, **kw: got.__setitem__(name, artifact), **kw)
        discrete = got["discrete_diarization"]
        off = np.asarray(discrete.data) > 0.5                            # Binarize at onset = offset = 0.5 on {0, 1} data
        Ko, Kl = off.shape[1], self.num_speakers
        T = min(len(off), self.covered)
        both = off[:T].astype(np.int64).T @ self.rows.valid("act")[:T, :Kl].astype(np.int64)     # [Ko, Kl] frames active in both
        labels = [-1] * Ko
        for i, j in zip(*linear_sum_assignment(-both)):
            labels[i] = int(j)
        fresh = Kl
        for i in range(Ko):
            if labels[i] < 0:
                labels[i], fresh = fresh, fresh + 1
        self.label_map = dict(enumerate(labels))
        if self.SCORES:
            self._final_scores = place_columns(np.asarray(got["speaker_scores"].data, dtype=np.float32), self.label_map, self.K)
        return activity_regions(off, discrete.sliding_window, uri=self.name, labels=labels)


def stream_live(pipeline, chunks: Iterable, sess_name: Optional[str] = None, recluster: bool = False, **kw
                ) -> Iterator[Tuple[float, float, Annotation]]:
    """generator form: chunks of float32 samples at the pipeline's rate (feed_format=: of the source's own bytes) -> (seconds received, committed seconds, Annotation)
    for every feed that produced an annotation, then the final triple.  scores=True: (seconds, committed seconds, Annotation,
    scores) — the session's `scores` after the feed, and `final_scores` on the same grid with the final Annotation"""
    sess = LiveDiarization(pipeline, sess_name, **kw)
    if not sess.SCORES:
        yield from stream_committed(sess, chunks, recluster=recluster)
        return
    for item in stream_committed(sess, chunks, recluster=recluster):
        yield item + (SlidingWindowFeature(sess.final_scores, sess.grid) if sess.finished else sess.scores,)
