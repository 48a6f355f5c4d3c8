"""Resegmentation — pyannote-audio 3.1.1's fourth pipeline over a segmentation model (PA/ = pyannote-audio/pyannote/audio/):

    Resegmentation              PA/pipelines/resegmentation.py:49-263     "given who speaks, redraw when each of them speaks"

It takes an existing diarization of a recording (from another system, a live session, coarse human labels, an older run) and
lets the segmentation model redraw its boundaries and overlaps; no embeddings, no clustering.  Only the segmentation forward
runs (as in detection.py: Inference(model) defaults, step 0.1 x duration, no median filter) and the decisions stay in HBM.
The one step the other pipelines do not have — matching the model's local speakers of every window to the speakers of the
given diarization, a Python loop over windows in the reference (resegmentation.py:230-243) — is one launch, dzn_match_counts
(csrc/reseg.hip): exact disagreement counts [C, n, n].  scipy's linear_sum_assignment then runs on the host over those, and
the speaker count, the aggregation of the matched decisions and the top-count selection are the calls the diarization pipeline
uses (postprocess.DevicePost).  With warm_up > 0 or more than 32 speakers the numpy composition (postprocess.resegment_host)
runs instead.

    reseg = Resegmentation.from_pretrained("path/to/hub_dir")            # or Resegmentation(diarizen_pipeline)
    refined = reseg("audio.wav", diarization=hypothesis)                 # Annotation, integer labels 0 .. n - 1
    named = identification.relabel(refined, dict(enumerate(reseg.labels)))

A powerset model emits hard {0,1} decisions, so the reference's binarize(onset, offset) (resegmentation.py:185-190) has nothing
to act on: onset / offset are refused by name, as detection.py does.  Labels of the result are the integer columns, as in the
reference (to_annotation gets a feature without labels); column k < K is the k-th label of the hypothesis sorted by str()
(`labels`), a column k >= K is a speaker the hypothesis did not have (possible only when it has fewer speakers than the model's
local ones).  Not pinned by a fixture of the reference: how the hypothesis is put on the frame grid
(postprocess.discretize_turns restates pyannote.core 5.0.0's Annotation.discretize), and tracks keep the column index where the
reference renames them "A", "B", ... (RTTM has no track field).
"""
from __future__ import annotations

import functools
import os
from pathlib import Path
from typing import Any, Callable, Dict, List, Mapping, Optional

import numpy as np
import torch

from . import dist as dz_dist
from .core import Annotation, SlidingWindowFeature
from .der import parse_rttm
from .detection import _Detection, _noop
from .postprocess import discretize_turns, receptive_field, reference_extent, resegment_device, trim_frames

PARAMETERS = ("warm_up", "min_duration_on", "min_duration_off")


def as_hypothesis(diarization, uri: Optional[str] = None):
    """an Annotation, RTTM text, the path of an RTTM file, or [(start, end, label)] -> what postprocess.discretize_turns takes
    (an Annotation or the list of turns).  RTTM lines of other recordings are skipped when the text names `uri` at all."""
    if diarization is None:
        raise ValueError('no diarization to refine: pass diarization=..., or a file mapping with a "diarization" key')
    if hasattr(diarization, "itertracks") or isinstance(diarization, (list, tuple)):
        return diarization
    if isinstance(diarization, os.PathLike) or (isinstance(diarization, str) and "\n" not in diarization
                                                and not diarization.lstrip().startswith("SPEAKER")):
        diarization = Path(diarization).read_text() if str(diarization) else ""
    if not isinstance(diarization, str):
        raise TypeError(f"diarization is an Annotation, RTTM text or a path, not {type(diarization).__name__}")
    turns = parse_rttm(diarization, uri) if uri is not None else []
    return turns or parse_rttm(diarization)


class Resegmentation(_Detection):
    """refine a given diarization with the segmentation model (module docstring).  Construction, from_pretrained,
    rttm_out_dir, resample=, channel= and close() are the detection pipelines'."""

    def __init__(self, segmentation, **kw):
        super().__init__(segmentation, **kw)
        self.warm_up = 0.0              # DiariZen's value (diarizen/pipelines/inference.py:138-142); pyannote's range is 0 .. 0.1
        self.labels: List = []          # the sorted labels of the last call's hypothesis: column k of the result is labels[k]

    # ------------------------------------------------------------------ hyper-parameters
    def instantiate(self, params: Dict[str, Any]):
        """warm_up: the ratio of every window trimmed on both sides before matching (Inference.trim; 0 <= warm_up < 0.5);
        min_duration_on / min_duration_off: Binarize's, seconds"""
        unknown = set(params) - set(PARAMETERS)
        if unknown:
            raise ValueError(f"unknown hyper-parameters {sorted(unknown)} (onset / offset do not exist for powerset models: "
                             "their decisions are hard already)")
        values = {k: float(v) for k, v in params.items()}
        w = values.get("warm_up", self.warm_up)
        if not 0.0 <= w < 0.5 or trim_frames(self._runner.num_frames, w)[1] < 1:
            raise ValueError(f"warm_up is a ratio in [0, 0.5) that leaves at least one frame, not {w!r}")
        for k, v in values.items():
            setattr(self, k, v)
        return self

    def parameters(self) -> Dict[str, float]:
        return {k: getattr(self, k) for k in PARAMETERS}

    def default_parameters(self) -> Dict[str, float]:
        return {"warm_up": 0.0, "min_duration_on": 0.0, "min_duration_off": 0.0}

    def classes(self):
        raise NotImplementedError("the speakers are those of the given diarization (resegmentation.py:131-132)")

    # ------------------------------------------------------------------ apply
    def apply(self, file, diarization=None, hook: Optional[Callable] = None):
        """file: what DiariZenPipeline.__call__ takes.  diarization: an Annotation, RTTM text or the path of an RTTM file;
        absent: file["diarization"].  An empty one is a hypothesis without speakers, not an error.
        hook(step_name, artifact, file=file, [completed=, total=]), the reference's steps (resegmentation.py:165-246):
        "segmentation" (progress, then the decisions [C, L, S]), "speaker_counting" [T, 1], "@resegmentation/original" (the
        hypothesis on the frame grid, u8 [Tr, K]), "@resegmentation/permutated" (hard int8 [C, S]: hard[c, j] = the column
        local speaker j of window c was matched to — not the dense array), "discrete_diarization" [T, n].
        -> Annotation with integer labels (module docstring), uri = file["uri"] or the path's stem; `labels` is set."""
        from .pipeline import open_recording, recording_on_device
        dz_dist.require_single_rank(type(self).__name__)
        file = file if isinstance(file, Mapping) else {"audio": file}
        audio = file["audio"]
        uri = file.get("uri")
        if uri is None and isinstance(audio, (str, os.PathLike)):
            uri = Path(audio).stem
        hypothesis = as_hypothesis(file.get("diarization") if diarization is None else diarization, uri)
        want = hook is not None
        hook = functools.partial(hook or _noop, file=file)            # Pipeline.setup_hook (PA/core/pipeline.py:267-271)
        x = open_recording(file, self.sample_rate, resample=self.resample, device=self.device, channel=self.channel)
        num_samples = int(x.num_samples) if hasattr(x, "num_samples") else len(x)
        chunks, frames = self.chunks_window(), receptive_field(self.sample_rate)
        _, Tr = reference_extent(num_samples, self.sample_rate, chunks, frames)
        ref, labels = discretize_turns(hypothesis, frames, Tr)
        with torch.cuda.device(self.device):
            wave = recording_on_device(x, self.device)
            res = self._runner.run(wave, with_embeddings=False,
                                   hook=functools.partial(hook, "segmentation", None) if want else None)
            seg_t = res.segmentations
            if want:
                hook("segmentation", SlidingWindowFeature(seg_t.cpu().numpy(), chunks))

            def step(name, artifact):
                if name == "speaker_counting":
                    hook("speaker_counting", artifact)
                    hook("@resegmentation/original", SlidingWindowFeature(ref, frames, labels))
                else:
                    hook("@resegmentation/permutated", artifact)
            _, _, _, discrete = resegment_device(seg_t, ref, chunks, frames, self.warm_up, step)
        hook("discrete_diarization", discrete)
        self.labels = list(labels)
        ann = self._regions(discrete.data, discrete.sliding_window, uri, None)
        self._write_rttm(ann, uri)
        return ann

    __call__ = apply

    # ------------------------------------------------------------------ live audio: out of scope
    def open_stream(self, *a, **kw):
        raise NotImplementedError("Resegmentation needs the whole hypothesis: it has no live form")

    open_hub = stream = open_stream


def annotation_from_discrete(discrete: SlidingWindowFeature, uri: Optional[str] = None, min_duration_on: float = 0.0,
                             min_duration_off: float = 0.0) -> Annotation:
    """to_annotation (PA/pipelines/utils/diarization.py:160-190) without a device: the discrete diarization [T, n] -> regions,
    then Binarize's min_duration_off / min_duration_on, exactly as detection._Detection._regions does"""
    shell = _Detection.__new__(_Detection)
    shell.min_duration_on, shell.min_duration_off = float(min_duration_on), float(min_duration_off)
    return shell._regions(np.asarray(discrete.data), discrete.sliding_window, uri, None)
