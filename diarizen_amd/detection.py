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

from . import dist as dz_dist
from .audio import Beamform, check_channel
from .core import SlidingWindow, SlidingWindowFeature
from .engine import Engine
from .inference import WindowRunner, window_plan
from .models import instantiate as instantiate_model
from .postprocess import (DETECT_OVERLAP, DETECT_SPEECH, _frame_grid, activity_regions, crop_end, detect_device,
                          detect_range_launch, detection_weights, receptive_field)
from .streaming import CommittedStream, stream_committed

ONSET = OFFSET = 0.5        # powerset models: fixed thresholds (voice_activity_detection.py:131, overlapped_speech_detection.py:138)
TASK_LABELS = {DETECT_SPEECH: "SPEECH", DETECT_OVERLAP: "OVERLAP"}


def _noop(*args, **kwargs):
    return


class _Detection:
    TASK = 0
    LABEL = ""

    def __init__(self, segmentation, *, rttm_out_dir: Optional[str] = None, device: Optional[torch.device] = None,
                 precision: str = "f32h", batch_size: Optional[int] = None, resample: Optional[str] = None,
                 channel=None):
        """segmentation: a DiariZen hub directory (config.toml + pytorch_model.bin; a segmentation-only engine is created,
        without the ResNet34 embedding model) or a `DiariZenPipeline`, whose engine handle(s) are reused (no second copy of
        the weights; its device and precision apply).  batch_size: windows per launch (default: the hub's
        [inference.args] batch_size, capped by the engine's max_batch).  resample: "host" | "device", where a recording at
        another rate is resampled (pipeline.open_recording; default: the DiariZenPipeline's setting, else "host").  channel: the
        channel of a recording that is read, an index, "downmix" or an audio.Beamform (default: the DiariZenPipeline's setting,
        else 0); a file mapping's "channel" key overrides it."""
        from .pipeline import DiariZenPipeline, _load_checkpoint, load_hub_config
        extra = ()
        self._owned: Optional[Engine] = None
        if resample is None:
            resample = segmentation.resample if isinstance(segmentation, DiariZenPipeline) else "host"
        if resample not in ("host", "device"):
            raise ValueError(f'resample is "host" or "device", not {resample!r}')
        self.resample = resample
        if channel is None:
            channel = segmentation.channel if isinstance(segmentation, DiariZenPipeline) else 0
        self.channel = channel if isinstance(channel, Beamform) else check_channel(channel)
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
        from .pipeline import open_recording, recording_on_device
        dz_dist.require_single_rank(type(self).__name__)
        file = file if isinstance(file, Mapping) else {"audio": file}
        audio = file["audio"]
        uri = file.get("uri")
        if uri is None and isinstance(audio, (str, os.PathLike)):
            uri = Path(audio).stem
        want_scores = hook is not None
        hook = functools.partial(hook or _noop, file=file)            # Pipeline.setup_hook (PA/core/pipeline.py:267-271)
        x = open_recording(file, self.sample_rate, resample=self.resample, device=self.device, channel=self.channel)
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
        max_seconds, slot_seconds, slots (the ingest ring, streaming.WaveIngest) and feed_format (an audio.FeedFormat: the
        feeds are the source's own bytes, G.711 or PCM frames at its rate, decoded and resampled on the device)."""
        return DetectionStream(self, uri=uri, tasks=tasks, scores=scores, **kw)

    def open_hub(self, max_sessions: int = 64, max_seconds: float = 600.0, slot_bytes: int = 1 << 20, slots: int = 4,
                 array_channels: int = 0, array_rate: Optional[int] = None):
        """many concurrent detection streams, one batched forward per tick: a hub.LiveHub whose `open(uri, ...)` takes the
        keywords of open_stream but the ingest's and returns a DetectionStream; `feed()` is then host work only and
        `hub.tick()` does the device work of every session at once.  max_sessions x max_seconds size ONE pooled device
        buffer (max_sessions x (max_seconds x rate + window) x 4 B), so max_seconds is far below a solo stream's 4 h.
        array_channels / array_rate: the most microphones and the highest feed rate of an array session (0: none are taken),
        as DiariZenPipeline.open_hub."""
        from .hub import LiveHub
        return LiveHub(self, lambda uri, hub, **kw: DetectionStream(self, uri=uri, hub=hub, **kw), max_sessions, max_seconds,
                       slot_bytes, slots, array_channels, array_rate)

    def stream(self, chunks: Iterable, uri: Optional[str] = None, **kw) -> Iterator[Tuple[float, float, Any]]:
        """generator form: chunks of float32 samples at the pipeline's rate (feed_format=: of the source's own bytes) -> (seconds received, committed seconds,
        Annotation) for every feed that produced an annotation, then the final triple (the offline result)"""
        yield from stream_committed(self.open_stream(uri=uri, **kw), chunks)


class VoiceActivityDetection(_Detection):
    """speech regions (label "SPEECH"): a frame scores 1 when at least one speaker is active in a window"""
    TASK = DETECT_SPEECH
    LABEL = "SPEECH"


class OverlappedSpeechDetection(_Detection):
    """overlapped speech regions (label "OVERLAP"): a frame scores 1 when at least two speakers are active in a window"""
    TASK = DETECT_OVERLAP
    LABEL = "OVERLAP"


class DetectionStream(CommittedStream):
    """Voice activity / overlapped speech detection on audio that is still arriving.

    The session is a streaming.CommittedStream (ingest, window schedule, frontier bookkeeping, feed / finish); the windows run
    through the detection pipeline's own runner (median filter off, no embeddings) once each, when their last sample has arrived.

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

    EMBEDDINGS = False

    def __init__(self, detection: _Detection, uri: Optional[str] = None, tasks: Optional[int] = None, scores: bool = False,
                 max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0, slots: int = 4, feed_format=None, hub=None):
        self.tasks = int(detection.TASK if tasks is None else tasks)
        if self.tasks & ~3 or not self.tasks & 3:
            raise ValueError(f"tasks is a bitmask of DETECT_SPEECH (1) and DETECT_OVERLAP (2), not {tasks!r}")
        self.labels = [TASK_LABELS[b] for b in (DETECT_SPEECH, DETECT_OVERLAP) if self.tasks & b]
        self.want_scores = bool(scores)
        K = len(self.labels)
        rows = {"act": (np.uint8, (K,))}
        if self.want_scores:
            rows["sc"] = (np.float32, (K,))
        super().__init__(detection, uri, rows, max_seconds, slot_seconds, slots, feed_format, hub)
        self.det = detection
        self.d_weight = torch.from_numpy(detection_weights(self.runner.num_frames, self.chunks.duration)).to(self.device)
        self._entry = None                                              # device u8 [K]: activity of frame frontier - 1

    @property
    def committed_activity(self) -> np.ndarray:
        """u8 [F, K]: the activity of the F committed frames (a copy)"""
        return self.rows.committed("act")

    @property
    def committed_scores(self) -> Optional[np.ndarray]:
        """f32 [F, K]: the aggregated scores of the committed frames (a copy), when the stream was opened with scores=True"""
        return self.rows.committed("sc") if self.want_scores else None

    def _range(self, t0: int, t1: int, frontier: int) -> dict:
        """one dzn_detect_range call; the activity of frame frontier - 1 is the next call's entry state"""
        sc, act = detect_range_launch(self.seg, self.done, self.d_start, self.d_weight, t0, t1, self.tasks,
                                      self.det.onset, self.det.offset, self._entry)
        if frontier > t0:
            self._entry = act[frontier - 1 - t0]
        return {"act": act, "sc": sc} if self.want_scores else {"act": act}

    def _annotate(self):
        return self.det._regions(self.rows.valid("act"), self.grid, self.name, self.labels)

    def _final_frames(self, T: int, has_last: bool) -> int:
        """the crop apply() makes after a zero-padded last window (PA/core/inference.py:400-403)"""
        return crop_end(T, self.grid, self.n / self.sr) if has_last else T

    def _write_rttm(self, ann) -> None:
        self.det._write_rttm(ann, self.name)
