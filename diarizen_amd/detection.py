"""VoiceActivityDetection / OverlappedSpeechDetection — the two other pipelines of pyannote-audio 3.1.1 that take a powerset
segmentation model (PA/ = pyannote-audio/pyannote/audio/):

    VoiceActivityDetection      PA/pipelines/voice_activity_detection.py:81-219     "where is speech"
    OverlappedSpeechDetection   PA/pipelines/overlapped_speech_detection.py:84-237  "where do two or more people talk at once"

with a DiariZen checkpoint as the segmentation model.  Only the segmentation forward runs (no embedding model, no
clustering): the recording is uploaded once, windows run through the engine (inference.WindowRunner, median filter off —
DiariZen's filter belongs to its diarization pipeline only), the decisions stay in HBM, and one dzn_detect call (csrc/post.hip)
aggregates them with the reference's Hamming-weighted float64/float32 arithmetic and applies the hysteresis.  Only the
[T] activity comes back (and the scores when a hook asks for them); the regions, the min_duration_on / min_duration_off
post-processing of Binarize (PA/utils/signal.py:207-317) and the RTTM are made on the host.

    vad = VoiceActivityDetection.from_pretrained("path/to/hub_dir")      # or VoiceActivityDetection(diarizen_pipeline)
    speech = vad("audio.wav")                                            # Annotation, label "SPEECH"

Live audio (DetectionStream): windows run as the samples arrive, and because detection needs no speaker labels the output has
a COMMITTED PREFIX — the offline bits, never revised — followed by a provisional tail one window long:

    for seconds, committed_seconds, speech in vad.stream(chunks, uri="meeting"):     # chunks: iterable of float32 arrays
        ...                                                              # final before committed_seconds, provisional after
"""
from __future__ import annotations

import functools
import math
import os
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, Iterator, Mapping, Optional, Tuple

import numpy as np
import torch

from .core import Annotation, SlidingWindow, SlidingWindowFeature
from .engine import Engine
from .inference import WindowRunner, window_plan
from .models import instantiate as instantiate_model
from .postprocess import (DETECT_OVERLAP, DETECT_SPEECH, _frame_grid, activity_regions, committed_frames, crop_end,
                          detect_device, detect_range_launch, detection_weights, receptive_field)

ONSET = OFFSET = 0.5        # powerset models: fixed thresholds (voice_activity_detection.py:131, overlapped_speech_detection.py:138)
TASK_LABELS = {DETECT_SPEECH: "SPEECH", DETECT_OVERLAP: "OVERLAP"}


def _noop(*args, **kwargs):
    return


class _Detection:
    TASK = 0
    LABEL = ""

    def __init__(self, segmentation, *, rttm_out_dir: Optional[str] = None, device: Optional[torch.device] = None,
                 precision: str = "f32h", batch_size: Optional[int] = None, resample: Optional[str] = None):
        """segmentation: a DiariZen hub directory (config.toml + pytorch_model.bin; a segmentation-only engine is created,
        without the ResNet34 embedding model) or a `DiariZenPipeline`, whose engine handle(s) are reused (no second copy of
        the weights; its device and precision apply).  batch_size: windows per launch (default: the hub's
        [inference.args] batch_size, capped by the engine's max_batch).  resample: "host" | "device", where a recording at
        another rate is resampled (pipeline.open_recording; default: the DiariZenPipeline's setting, else "host")."""
        from .pipeline import DiariZenPipeline, _load_checkpoint, load_hub_config
        extra = ()
        self._owned: Optional[Engine] = None
        if resample is None:
            resample = segmentation.resample if isinstance(segmentation, DiariZenPipeline) else "host"
        if resample not in ("host", "device"):
            raise ValueError(f'resample is "host" or "device", not {resample!r}')
        self.resample = resample
        if isinstance(segmentation, DiariZenPipeline):
            pipe = segmentation
            self.device = pipe.device
            self.segmentation_model = pipe.segmentation_model
            self.engine = pipe.engine
            extra = pipe.extra_engines
            bs = int(batch_size or pipe.batch_size)
        else:
            if not torch.cuda.is_available():
                raise RuntimeError(f"{type(self).__name__} (diarizen_amd) needs a HIP device; no CPU fallback")
            hub = Path(segmentation)
            config = load_hub_config(hub)
            self.device = torch.device(device or "cuda:0")
            bs = int(batch_size or config.get("inference", {}).get("args", {}).get("batch_size", 32))
            margs = dict(config["model"]["args"])
            margs.setdefault("precision", precision)
            margs["max_batch"] = bs
            self.segmentation_model = instantiate_model(config["model"]["path"], margs)
            seg_state = _load_checkpoint(str(hub / "pytorch_model.bin"))
            window = int(math.floor(self.segmentation_model.specifications.duration * self.segmentation_model.sample_rate))
            self.engine = self._owned = Engine(self.segmentation_model.cfg, seg_state, None, None, max_batch=bs,
                                               max_samples=window, precision=precision, device=self.device)
            self.segmentation_model.load_state_dict(seg_state).bind(self.engine)
        assert self.segmentation_model.specifications.powerset is True, "only powerset segmentation models"
        self.sample_rate = self.segmentation_model.sample_rate
        # Inference(model) defaults (PA/core/inference.py:83-182): window = specifications.duration, step = 0.1 x window
        self.duration = float(self.segmentation_model.specifications.duration)
        self._runner = WindowRunner(self.engine, self.duration, 0.1, bs, median_size=0, exclude_overlap=False,
                                    sample_rate=self.sample_rate, extra_engines=tuple(extra))
        self.onset = self.offset = ONSET
        self.min_duration_on = 0.0
        self.min_duration_off = 0.0
        if rttm_out_dir is not None:
            os.makedirs(rttm_out_dir, exist_ok=True)
        self.rttm_out_dir = rttm_out_dir

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, repo_id: str, cache_dir: Optional[str] = None, rttm_out_dir: Optional[str] = None, **kw):
        """repo_id: a local hub directory or an HF hub id, resolved as `DiariZenPipeline.from_pretrained` does"""
        from .pipeline import resolve_hub
        return cls(resolve_hub(repo_id, cache_dir), rttm_out_dir=rttm_out_dir, **kw)

    def instantiate(self, params: Dict[str, Any]):
        """pyannote.pipeline's instantiate: the two hyper-parameters of a powerset model's detection pipeline
        (min_duration_on: remove regions shorter than that; min_duration_off: fill gaps shorter than that; seconds)"""
        unknown = set(params) - {"min_duration_on", "min_duration_off"}
        if unknown:
            raise ValueError(f"unknown hyper-parameters {sorted(unknown)} (onset / offset are fixed at 0.5 for powerset models)")
        for k, v in params.items():
            setattr(self, k, float(v))
        return self

    def parameters(self) -> Dict[str, float]:
        return {"min_duration_on": self.min_duration_on, "min_duration_off": self.min_duration_off}

    def default_parameters(self) -> Dict[str, float]:
        return {"min_duration_on": 0.0, "min_duration_off": 0.0}       # segmentation-3.0 (voice_activity_detection.py:152-156)

    def classes(self):
        return [self.LABEL]

    def close(self) -> None:
        """release the segmentation-only engine this pipeline created (an engine borrowed from a DiariZenPipeline stays)"""
        self._runner.close()
        if self._owned is not None:
            self._owned.close()
            self._owned = None

    # ------------------------------------------------------------------ apply
    def chunks_window(self) -> SlidingWindow:
        return SlidingWindow(start=0.0, duration=self.duration, step=0.1 * self.duration)

    def apply(self, file, hook: Optional[Callable] = None):
        """file: what DiariZenPipeline.__call__ takes (path, BytesIO, bytes, or a mapping with "audio" and optionally "uri").
        hook(step_name, artifact, file=file, [completed=, total=]): "segmentation" progress per batch of windows, then the
        aggregated scores as a SlidingWindowFeature [T, 1] (PA/pipelines/voice_activity_detection.py:188-214).
        -> Annotation of the regions, labelled "SPEECH" / "OVERLAP", uri = file["uri"] or the path's stem."""
        from . import dist as dz_dist
        from .pipeline import open_recording, recording_on_device
        if dz_dist.world_size() > 1:
            raise RuntimeError(f"{type(self).__name__} runs on one device: sharding a recording over torch.distributed ranks "
                               f"is not supported (world size {dz_dist.world_size()})")
        file = file if isinstance(file, Mapping) else {"audio": file}
        audio = file["audio"]
        uri = file.get("uri")
        if uri is None and isinstance(audio, (str, os.PathLike)):
            uri = Path(audio).stem
        want_scores = hook is not None
        hook = functools.partial(hook or _noop, file=file)            # Pipeline.setup_hook (PA/core/pipeline.py:267-271)
        x = open_recording(audio, self.sample_rate, resample=self.resample, device=self.device)
        n = int(x.num_samples) if hasattr(x, "num_samples") else len(x)
        with torch.cuda.device(self.device):
            wave = recording_on_device(x, self.device)
            res = self._runner.run(wave, with_embeddings=False,
                                   hook=functools.partial(hook, "segmentation", None) if want_scores else None)
            chunks, frames = self.chunks_window(), receptive_field(self.sample_rate)
            C, L, _ = res.segmentations.shape
            grid, _, T = _frame_grid(C, L, chunks, frames)
            if window_plan(n, self._runner.window, self._runner.step)[1]:
                T = crop_end(T, grid, n / self.sample_rate)          # zero-padded last window: PA/core/inference.py:400-403
            active, scores, grid = detect_device(res.segmentations, chunks, frames, self.TASK, num_frames=T,
                                                 onset=self.onset, offset=self.offset, want_scores=want_scores)
        if want_scores:
            hook("segmentation", SlidingWindowFeature(scores, grid))
        ann = self._regions(active, grid, uri, [self.LABEL])
        self._write_rttm(ann, uri)
        return ann

    __call__ = apply

    def _regions(self, active: np.ndarray, grid: SlidingWindow, uri: Optional[str], labels):
        """per-frame activity [n, K] -> Annotation: the regions, then Binarize's post-processing"""
        ann = activity_regions(active.astype(bool), grid, uri=uri, labels=labels)
        # Binarize's post-processing (PA/utils/signal.py:302-315): fill short gaps, then drop short regions
        if self.min_duration_off > 0.0:
            ann = ann.support(collar=self.min_duration_off)
        if self.min_duration_on > 0.0:
            for segment, track in list(ann.itertracks()):
                if segment.duration < self.min_duration_on:
                    del ann[segment, track]
        ann.uri = uri
        return ann

    def _write_rttm(self, ann, uri: Optional[str]) -> None:
        if self.rttm_out_dir is not None:
            if uri is None:
                raise ValueError("rttm_out_dir needs a uri: pass {'audio': ..., 'uri': ...} for in-memory audio")
            with open(os.path.join(self.rttm_out_dir, f"{uri}.rttm"), "w") as f:
                f.write(ann.to_rttm())

    # ------------------------------------------------------------------ live audio
    def open_stream(self, uri: Optional[str] = None, tasks: Optional[int] = None, scores: bool = False, **kw) -> "DetectionStream":
        """push form for audio that is still arriving: `DetectionStream.feed(samples)` / `.finish()`.  tasks: the dzn_detect
        bitmask (DETECT_SPEECH | DETECT_OVERLAP gives both detections from one pass over the windows, one label per column;
        default: this pipeline's own task).  scores: also keep the aggregated scores (`committed_scores`).  Further keywords:
        max_seconds, slot_seconds, slots (the ingest ring, streaming.WaveIngest)."""
        return DetectionStream(self, uri=uri, tasks=tasks, scores=scores, **kw)

    def stream(self, chunks: Iterable, uri: Optional[str] = None, **kw) -> Iterator[Tuple[float, float, Any]]:
        """generator form: chunks of float32 samples at the pipeline's rate -> (seconds received, committed seconds,
        Annotation) for every feed that produced an annotation, then the final triple (the offline result)"""
        sess = self.open_stream(uri=uri, **kw)
        for c in chunks:
            ann = sess.feed(c)
            if ann is not None:
                yield sess.seconds, sess.committed_seconds, ann
        ann = sess.finish()
        yield sess.seconds, sess.committed_seconds, ann


class VoiceActivityDetection(_Detection):
    """speech regions (label "SPEECH"): a frame scores 1 when at least one speaker is active in a window"""
    TASK = DETECT_SPEECH
    LABEL = "SPEECH"


class OverlappedSpeechDetection(_Detection):
    """overlapped speech regions (label "OVERLAP"): a frame scores 1 when at least two speakers are active in a window"""
    TASK = DETECT_OVERLAP
    LABEL = "OVERLAP"


class DetectionStream:
    """Voice activity / overlapped speech detection on audio that is still arriving.

    Ingest is the streaming session's (streaming.WaveIngest: pinned host ring, copy stream, one pre-zeroed device buffer whose
    windows are rows of a strided view); the windows run through the detection pipeline's own runner (median filter off, no
    embeddings) once each, when their last sample has arrived, and their u8 decisions are kept in one device buffer.

    A frame's aggregated score depends only on the windows that cover it, and window start frames do not depend on how many
    windows exist.  With windows 0 .. C - 1 computed, every frame before the start frame of window C (the FRONTIER,
    postprocess.committed_frames) therefore has its final score, and — the hysteresis being a left-to-right scan — its final
    activity: `committed_activity` / `committed_scores` are the offline bits and only ever grow.  Frames from the frontier to
    the end of window C - 1 are the provisional tail; the next window revises them.  Per feed one dzn_detect_range call computes
    [previous frontier, frames covered so far) with the committed activity of the frame before it as the entry state — nothing
    that is already final is derived again.

    feed() returns None until the first window is complete, then an Annotation over every frame computed so far.  With
    min_duration_on / min_duration_off set, provisional annotations get the same post-processing as the final one; it acts on
    regions, not frames, so the region or gap that touches the frontier may still change (a short gap there may yet be filled, a
    short region there may yet grow) — only the per-frame arrays are final.  finish() gives what apply() gives on the whole
    recording."""

    def __init__(self, detection: _Detection, uri: Optional[str] = None, tasks: Optional[int] = None, scores: bool = False,
                 max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0, slots: int = 4):
        from . import dist as dz_dist
        from .streaming import WaveIngest
        if dz_dist.world_size() > 1:
            raise RuntimeError(f"{type(self).__name__} runs on one device: sharding a recording over torch.distributed ranks "
                               f"is not supported (world size {dz_dist.world_size()})")
        self.det = detection
        self.uri = uri
        self.tasks = int(detection.TASK if tasks is None else tasks)
        if self.tasks & ~3 or not self.tasks & 3:
            raise ValueError(f"tasks is a bitmask of DETECT_SPEECH (1) and DETECT_OVERLAP (2), not {tasks!r}")
        self.labels = [TASK_LABELS[b] for b in (DETECT_SPEECH, DETECT_OVERLAP) if self.tasks & b]
        self.want_scores = bool(scores)
        r = detection._runner
        self.runner = r
        self.sr = r.sample_rate
        self.device = dev = detection.device
        self.chunks, self.frames = detection.chunks_window(), receptive_field(self.sr)
        with torch.cuda.device(dev):
            self.ingest = WaveIngest(dev, self.sr, r.window, r.step, max_seconds, slot_seconds, slots)
            cmax = self.ingest.views.shape[0]
            L, S = r.num_frames, detection.engine.seg.max_speakers_per_chunk
            self.grid, starts, _ = _frame_grid(cmax, L, self.chunks, self.frames)
            self.seg = torch.zeros((cmax, L, S), device=dev, dtype=torch.uint8)       # decisions of every window so far
            self.d_start = torch.from_numpy(starts).to(dev)
            self.d_weight = torch.from_numpy(detection_weights(L, self.chunks.duration)).to(dev)
        K = len(self.labels)
        self.done = 0                                                   # windows computed
        self.frontier = 0                                               # frames committed
        self.covered = 0                                                # frames computed (committed + provisional tail)
        self._act = np.zeros((1024, K), dtype=np.uint8)                 # rows < frontier final, rows < covered valid
        self._sc = np.zeros((1024, K), dtype=np.float32) if self.want_scores else None
        self._entry = None                                              # device u8 [K]: activity of frame frontier - 1
        self._last = None
        self.finished = False
        self.stats = {"uploads": 0, "windows": 0, "launches": 0, "range_calls": 0}

    # ------------------------------------------------------------------ state
    @property
    def n(self) -> int:
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
    def committed_activity(self) -> np.ndarray:
        """u8 [F, K]: the activity of the F committed frames (a copy)"""
        return self._act[:self.frontier].copy()

    @property
    def committed_scores(self) -> Optional[np.ndarray]:
        """f32 [F, K]: the aggregated scores of the committed frames (a copy), when the stream was opened with scores=True"""
        return self._sc[:self.frontier].copy() if self.want_scores else None

    def _covered_frames(self, num_windows: int) -> int:
        """number of frames Inference.aggregate gives for `num_windows` windows (as _frame_grid)"""
        c, g = self.chunks, self.grid
        return int(g.closest_frame(c.start + c.duration + (num_windows - 1) * c.step + 0.5 * g.duration) + 1)

    # ------------------------------------------------------------------ device work
    def _compute(self, upto: int) -> None:
        """run windows done .. upto behind the newest upload and append their decisions to the device buffer"""
        if upto <= self.done:
            return
        self.ingest.wait()
        res = self.runner.run_views(self.ingest.views, self.done, upto, with_embeddings=False)
        self.seg[self.done:upto] = res.segmentations
        self.stats["windows"] += upto - self.done
        self.stats["launches"] += 1
        self.done = upto

    def _detect(self, upto_frames: int, frontier: int) -> None:
        """one range call over [self.frontier, upto_frames); frames below `frontier` are committed"""
        t0, t1 = self.frontier, max(int(upto_frames), self.frontier)
        frontier = min(max(frontier, t0), t1)
        if t1 > len(self._act):
            cap = max(t1, 2 * len(self._act))
            self._act = np.concatenate([self._act, np.zeros((cap - len(self._act), self._act.shape[1]), np.uint8)])
            if self.want_scores:
                self._sc = np.concatenate([self._sc, np.zeros((cap - len(self._sc), self._sc.shape[1]), np.float32)])
        if t1 > t0:
            sc, act = detect_range_launch(self.seg, self.done, self.d_start, self.d_weight, t0, t1, self.tasks,
                                          self.det.onset, self.det.offset, self._entry)
            self.stats["range_calls"] += 1
            self._act[t0:t1] = act.cpu().numpy()
            if self.want_scores:
                self._sc[t0:t1] = sc.cpu().numpy()
            if frontier > t0:
                self._entry = act[frontier - 1 - t0]
        self.frontier, self.covered = frontier, t1

    def _annotate(self):
        return self.det._regions(self._act[:self.covered], self.grid, self.uri, self.labels)

    # ------------------------------------------------------------------ feed / finish
    def feed(self, samples):
        """append float32 samples (mono, the pipeline's rate).  -> None while no window is complete, else the Annotation over
        every frame computed so far (final before `committed_seconds`, provisional after)"""
        from .streaming import complete_windows
        if self.finished:
            raise RuntimeError("stream already finished")
        with torch.cuda.device(self.device):
            taken = self.ingest.append(samples)
            self.stats["uploads"] = self.ingest.uploads
            upto = complete_windows(self.ingest.n, self.runner.window, self.runner.step)
            if taken and upto > self.done:
                self._compute(upto)
                self._detect(self._covered_frames(self.done), committed_frames(self.done, self.chunks, self.frames))
                self._last = self._annotate()
        return self._last

    def finish(self):
        """end of stream: the zero-padded last window if the reference would run one, the crop apply() makes, everything
        committed -> the Annotation apply() gives on the whole recording (and its RTTM file when rttm_out_dir is set)"""
        if self.finished:
            raise RuntimeError("stream already finished")
        r = self.runner
        n = self.ingest.n
        n_full, has_last = window_plan(n, r.window, r.step)
        self.finished = True
        if n == 0:
            return Annotation(uri=self.uri)
        with torch.cuda.device(self.device):
            self._compute(n_full + int(has_last))
            T = self._covered_frames(self.done)
            if has_last:
                T = crop_end(T, self.grid, n / self.sr)          # zero-padded last window: PA/core/inference.py:400-403
            assert self.frontier <= T, "committed frames beyond the offline output"
            self._detect(T, T)
        ann = self._last = self._annotate()
        self.det._write_rttm(ann, self.uri)
        return ann
