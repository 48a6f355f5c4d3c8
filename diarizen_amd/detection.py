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
"""
from __future__ import annotations

import functools
import math
import os
from pathlib import Path
from typing import Any, Callable, Dict, Mapping, Optional

import numpy as np
import torch

from .core import SlidingWindow, SlidingWindowFeature
from .engine import Engine
from .inference import WindowRunner, window_plan
from .models import instantiate as instantiate_model
from .postprocess import (DETECT_OVERLAP, DETECT_SPEECH, _frame_grid, activity_regions, crop_end, detect_device,
                          receptive_field)

ONSET = OFFSET = 0.5        # powerset models: fixed thresholds (voice_activity_detection.py:131, overlapped_speech_detection.py:138)


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
        ann = activity_regions(active.astype(bool), grid, uri=uri, labels=[self.LABEL])
        # Binarize's post-processing (PA/utils/signal.py:302-315): fill short gaps, then drop short regions
        if self.min_duration_off > 0.0:
            ann = ann.support(collar=self.min_duration_off)
        if self.min_duration_on > 0.0:
            for segment, track in list(ann.itertracks()):
                if segment.duration < self.min_duration_on:
                    del ann[segment, track]
        ann.uri = uri
        if self.rttm_out_dir is not None:
            if uri is None:
                raise ValueError("rttm_out_dir needs a uri: pass {'audio': ..., 'uri': ...} for in-memory audio")
            with open(os.path.join(self.rttm_out_dir, f"{uri}.rttm"), "w") as f:
                f.write(ann.to_rttm())
        return ann

    __call__ = apply


class VoiceActivityDetection(_Detection):
    """speech regions (label "SPEECH"): a frame scores 1 when at least one speaker is active in a window"""
    TASK = DETECT_SPEECH
    LABEL = "SPEECH"


class OverlappedSpeechDetection(_Detection):
    """overlapped speech regions (label "OVERLAP"): a frame scores 1 when at least two speakers are active in a window"""
    TASK = DETECT_OVERLAP
    LABEL = "OVERLAP"
