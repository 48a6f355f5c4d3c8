"""Live speaker diarization: who is speaking now, under a label that does not change.

    live = pipeline.open_live(sess_name="meeting")
    for chunk in microphone:                               # float32 arrays at the pipeline's rate
        ann = live.feed(chunk)                             # None until the first window is complete
        ...                                                # final before live.committed_seconds, provisional after
    ann = live.finish()                                    # or finish(recluster=True): the offline result under the live labels

    for seconds, committed_seconds, ann in pipeline.stream_live(chunks, sess_name="meeting"): ...

The shape is detection.DetectionStream's: ingest is streaming.WaveIngest, every window runs ONCE through the pipeline's own
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
number of frames in which both are active)."""
from __future__ import annotations

import os
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np
import torch

from .core import Annotation
from .inference import window_plan
from .online import OnlineSpeakers
from .postprocess import _frame_grid, activity_regions, committed_frames, diarize_range_launch, receptive_field
from .streaming import WaveIngest, complete_windows


class LiveDiarization:
    def __init__(self, pipeline, sess_name: Optional[str] = None, delta_new: Optional[float] = None,
                 max_speakers: Optional[int] = None, max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0,
                 slots: int = 4):
        """delta_new: the distance beyond which a clean local speaker opens a new label (default: the pipeline's
        ahc_threshold); max_speakers: the cap on labels (default: the pipeline's, at most 32); max_seconds, slot_seconds,
        slots: the ingest ring (streaming.WaveIngest)."""
        from . import dist as dz_dist
        if dz_dist.world_size() > 1:
            raise RuntimeError(f"{type(self).__name__} runs on one device: sharding a recording over torch.distributed ranks "
                               f"is not supported (world size {dz_dist.world_size()})")
        self.pipe = pipeline
        self.sess_name = sess_name
        r = pipeline._runner
        self.runner = r
        self.sr = r.sample_rate
        self.device = dev = pipeline.device
        self.K = min(int(max_speakers or pipeline.max_speakers), 32)
        if self.K < 1:
            raise ValueError(f"max_speakers must be at least 1, not {max_speakers!r}")
        if delta_new is None:
            delta_new = pipeline.config["clustering"]["args"]["ahc_threshold"]
        self.chunks, self.frames = pipeline.chunks_window(), receptive_field(self.sr)
        with torch.cuda.device(dev):
            self.ingest = WaveIngest(dev, self.sr, r.window, r.step, max_seconds, slot_seconds, slots)
            cmax = self.ingest.views.shape[0]
            L, S = r.num_frames, pipeline.engine.seg.max_speakers_per_chunk
            self.grid, starts, _ = _frame_grid(cmax, L, self.chunks, self.frames)
            self.seg = torch.zeros((cmax, L, S), device=dev, dtype=torch.uint8)       # decisions of every window so far
            self.hard = torch.full((cmax, S), -2, device=dev, dtype=torch.int8)       # their global labels
            self.d_start = torch.from_numpy(starts).to(dev)
        self.speakers = OnlineSpeakers(delta_new, self.K, pipeline.engine.emb.embed_dim)
        self.done = 0                                                   # windows computed and labelled
        self.frontier = 0                                               # frames committed
        self.covered = 0                                                # frames computed (committed + provisional tail)
        self._seg_h, self._emb_h = [], []                               # per feed: the new windows' decisions / embeddings (host)
        self._hard_h = np.zeros((0, S), dtype=np.int8)
        self._act = np.zeros((1024, self.K), dtype=np.uint8)            # rows < frontier final, rows < covered valid
        self._cnt = np.zeros(1024, dtype=np.uint8)
        self._last = None
        self.label_map = None                                           # finish(recluster=True): offline cluster -> live label
        self.finished = False
        self.stats = {"uploads": 0, "windows": 0, "launches": 0, "range_calls": 0}

    # ------------------------------------------------------------------ state
    @property
    def n(self) -> int:
        """samples received"""
        return self.ingest.n

    @property
    def seconds(self) -> float:
        """seconds of audio received"""
        return self.ingest.n / self.sr

    @property
    def committed_seconds(self) -> float:
        """start time of the first frame that may still change"""
        return self.grid.start + self.frontier * self.grid.step

    @property
    def committed_diarization(self) -> np.ndarray:
        """u8 [F, K]: the speaker activity of the F committed frames, column k = label k (a copy)"""
        return self._act[:self.frontier].copy()

    @property
    def committed_count(self) -> np.ndarray:
        """u8 [F]: the (capped) instantaneous speaker count of the committed frames (a copy)"""
        return self._cnt[:self.frontier].copy()

    @property
    def num_speakers(self) -> int:
        """labels opened so far"""
        return self.speakers.num_speakers

    @property
    def hard_clusters(self) -> np.ndarray:
        """int8 [done, S]: the label of every local speaker of every window so far, -2 = none (a copy)"""
        return self._hard_h.copy()

    def _covered_frames(self, num_windows: int) -> int:
        """number of frames Inference.aggregate gives for `num_windows` windows (as _frame_grid)"""
        c, g = self.chunks, self.grid
        return int(g.closest_frame(c.start + c.duration + (num_windows - 1) * c.step + 0.5 * g.duration) + 1)

    # ------------------------------------------------------------------ device / host work
    def _compute(self, upto: int) -> None:
        """run windows done .. upto behind the newest upload, keep their decisions on the device, label them on the host
        and upload the new rows of the hard buffer"""
        if upto <= self.done:
            return
        self.ingest.wait()
        res = self.runner.run_views(self.ingest.views, self.done, upto, with_embeddings=True)
        self.seg[self.done:upto] = res.segmentations
        seg, emb = res.segmentations.cpu().numpy(), res.embeddings.cpu().numpy()      # the new windows only
        hard = np.stack([self.speakers.assign(seg[i], emb[i]) for i in range(upto - self.done)])
        self.hard[self.done:upto] = torch.from_numpy(hard).to(self.device)
        self._seg_h.append(seg)
        self._emb_h.append(emb)
        self._hard_h = np.concatenate([self._hard_h, hard])
        self.stats["windows"] += upto - self.done
        self.stats["launches"] += 1
        self.done = upto

    def _diarize(self, upto_frames: int, frontier: int) -> None:
        """one range call over [self.frontier, upto_frames); frames below `frontier` are committed"""
        t0, t1 = self.frontier, max(int(upto_frames), self.frontier)
        frontier = min(max(frontier, t0), t1)
        if t1 > len(self._act):
            cap = max(t1, 2 * len(self._act))
            self._act = np.concatenate([self._act, np.zeros((cap - len(self._act), self.K), np.uint8)])
            self._cnt = np.concatenate([self._cnt, np.zeros(cap - len(self._cnt), np.uint8)])
        if t1 > t0:
            cnt, act, _ = diarize_range_launch(self.seg, self.hard, self.done, self.d_start, t0, t1, self.K, self.K)
            self.stats["range_calls"] += 1
            self._act[t0:t1] = act.cpu().numpy()
            self._cnt[t0:t1] = cnt.cpu().numpy()
        self.frontier, self.covered = frontier, t1

    def _annotate(self) -> Annotation:
        return activity_regions(self._act[:self.covered].astype(bool), self.grid, uri=self.sess_name)

    # ------------------------------------------------------------------ feed / finish
    def feed(self, samples) -> Optional[Annotation]:
        """append float32 samples (mono, the pipeline's rate).  -> None while no window is complete, else the Annotation over
        every frame computed so far, integer labels as offline (final before `committed_seconds`, label included; the tail of
        one window after it is provisional)"""
        if self.finished:
            raise RuntimeError("stream already finished")
        with torch.cuda.device(self.device):
            taken = self.ingest.append(samples)
            self.stats["uploads"] = self.ingest.uploads
            upto = complete_windows(self.ingest.n, self.runner.window, self.runner.step)
            if taken and upto > self.done:
                self._compute(upto)
                self._diarize(self._covered_frames(self.done), committed_frames(self.done, self.chunks, self.frames))
                self._last = self._annotate()
        return self._last

    def finish(self, recluster: bool = False) -> Annotation:
        """end of stream: the zero-padded last window if the reference would run one, every frame committed (no crop at the
        end of the audio: the offline Annotation has none) -> the final Annotation, and its RTTM file when the pipeline has an
        rttm_out_dir and the session a name.
        recluster=True: the ordinary host stage (counting, AHC / VBx with min_cluster_size, reconstruction) over all windows;
        its clusters are matched to the live speakers (linear_sum_assignment, maximising the frames in which both are active;
        offline clusters left over get fresh labels from `num_speakers` upward) and ITS annotation is returned under the live
        labels; `label_map` keeps offline cluster -> live label.  The committed arrays stay the live ones."""
        if self.finished:
            raise RuntimeError("stream already finished")
        r = self.runner
        n = self.ingest.n
        n_full, has_last = window_plan(n, r.window, r.step)
        self.finished = True
        if n == 0:
            return Annotation(uri=self.sess_name)
        with torch.cuda.device(self.device):
            self._compute(n_full + int(has_last))
            T = self._covered_frames(self.done)
            self._diarize(T, T)
        ann = self._recluster() if recluster else self._annotate()
        self._last = ann
        if self.pipe.rttm_out_dir is not None and self.sess_name is not None:
            with open(os.path.join(self.pipe.rttm_out_dir, self.sess_name + ".rttm"), "w") as f:
                f.write(ann.to_rttm())
        return ann

    def _recluster(self) -> Annotation:
        from scipy.optimize import linear_sum_assignment
        got = {}
        self.pipe.host_stage(np.concatenate(self._seg_h), np.concatenate(self._emb_h), self.sess_name,
                             hook=lambda name, artifact, **kw: got.__setitem__(name, artifact))
        discrete = got["discrete_diarization"]
        off = np.asarray(discrete.data) > 0.5                            # Binarize at onset = offset = 0.5 on {0, 1} data
        Ko, Kl = off.shape[1], self.num_speakers
        T = min(len(off), self.covered)
        both = off[:T].astype(np.int64).T @ self._act[:T, :Kl].astype(np.int64)       # [Ko, Kl] frames active in both
        labels = [-1] * Ko
        for i, j in zip(*linear_sum_assignment(-both)):
            labels[i] = int(j)
        fresh = Kl
        for i in range(Ko):
            if labels[i] < 0:
                labels[i], fresh = fresh, fresh + 1
        self.label_map = dict(enumerate(labels))
        return activity_regions(off, discrete.sliding_window, uri=self.sess_name, labels=labels)


def stream_live(pipeline, chunks: Iterable, sess_name: Optional[str] = None, recluster: bool = False, **kw
                ) -> Iterator[Tuple[float, float, Annotation]]:
    """generator form: chunks of float32 samples at the pipeline's rate -> (seconds received, committed seconds, Annotation)
    for every feed that produced an annotation, then the final triple"""
    sess = LiveDiarization(pipeline, sess_name, **kw)
    for c in chunks:
        ann = sess.feed(c)
        if ann is not None:
            yield sess.seconds, sess.committed_seconds, ann
    ann = sess.finish(recluster=recluster)
    yield sess.seconds, sess.committed_seconds, ann
