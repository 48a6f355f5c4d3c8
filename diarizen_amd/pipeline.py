"""DiariZenPipeline — drop-in for diarizen/pipelines/inference.py:26-192.

Same public surface: `DiariZenPipeline.from_pretrained(repo_id, cache_dir=None, rttm_out_dir=None)`
and `pipeline(in_wav, sess_name=None) -> Annotation` (+ RTTM file), same hub directory layout
(`config.toml`, `pytorch_model.bin`, `plda/`), same `[inference.args]` / `[clustering.args]` keys.
What changes is where the time goes: the recording is uploaded once, every window runs
segmentation -> masks -> embeddings on the MI355X through libdzn_hip.so (diarizen_amd/inference.py),
windows can be sharded over the GPUs of a node (diarizen_amd/dist.py), and the host only sees
u8 decisions + f32 embeddings for counting / clustering / reconstruction (diarizen_amd/postprocess.py,
diarizen_amd/clustering.py), which follow the reference arithmetic so the RTTM is equal.
"""
from __future__ import annotations

import os
from io import BytesIO
from pathlib import Path
from typing import Any, Dict, Mapping, Optional

import numpy as np
import torch

from . import audio as audio_io
from .clustering import AgglomerativeClustering, VBxClustering, active_speakers
from .configs import RESNET34
from .core import Annotation, SlidingWindow, SlidingWindowFeature
from .engine import Engine
from .inference import WindowRunner, window_plan
from .models import SpeakerEmbedding, WavLMConformer, instantiate
from .postprocess import (DevicePost, _frame_grid, binarize, crop_end, receptive_field, reconstruct, speaker_count,
                          speaker_scores)

try:
    import tomllib as _toml  # py311+
except ImportError:  # pragma: no cover
    import tomli as _toml

EMBEDDING_REPO = "pyannote/wespeaker-voxceleb-resnet34-LM"


def _lightning_safe_globals():
    """non-tensor globals the known Lightning checkpoints carry (pyannote/wespeaker-voxceleb-resnet34-LM pickles a
    `TorchVersion` in its `pyannote.audio` version block; hyper-parameter blocks use plain containers), allow-listed so
    that the tensors-only unpickler loads them — nothing here executes code on load"""
    import collections
    allow = [collections.OrderedDict, collections.defaultdict, dict, list, tuple, set, frozenset, complex, slice]
    try:
        from torch.torch_version import TorchVersion
        allow.append(TorchVersion)
    except Exception:       # pragma: no cover
        pass
    return allow


def _load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """plain state_dict (DiariZen hub `pytorch_model.bin`) or Lightning checkpoint (WeSpeaker, PA/core/model.py:459-473).
    Always the tensors-only unpickler: first as is, then with the known Lightning globals allow-listed (the real
    pyannote/WeSpeaker checkpoint holds a `TorchVersion`, which `weights_only=True` rejects on its own — the breakage
    pyannote hit with torch 2.6).  The permissive unpickler is an explicit opt-in (DZN_TRUST_CHECKPOINTS=1), never a
    silent fallback."""
    import pickle
    first = None
    ckpt = None
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, TypeError) as e:
        first = e
    if ckpt is None:
        try:
            with torch.serialization.safe_globals(_lightning_safe_globals()):
                ckpt = torch.load(path, map_location="cpu", weights_only=True)
        except (pickle.UnpicklingError, RuntimeError, TypeError, AttributeError) as e:
            if os.environ.get("DZN_TRUST_CHECKPOINTS") != "1":
                raise RuntimeError(f"{path}: not loadable with the tensors-only unpickler ({type(first).__name__}: {first}; with "
                                   f"the Lightning allow-list: {type(e).__name__}: {e}).  If this file comes from a source you "
                                   f"trust, set DZN_TRUST_CHECKPOINTS=1 to load it with the full unpickler.") from None
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(ckpt, dict) and "state_dict" in ckpt and isinstance(ckpt["state_dict"], dict):
        ckpt = ckpt["state_dict"]          # Lightning checkpoint (PA/core/model.py:459-473)
    return ckpt


def run_host_stage(seg: np.ndarray, emb: np.ndarray, *, chunks: SlidingWindow, clustering, min_speakers: int,
                   max_speakers: int, sample_rate: int = 16000, sess_name: Optional[str] = None,
                   device=None, hook=None, soft=None, num_frames: Optional[int] = None, return_embeddings: bool = False):
    """The host half of `DiariZenPipeline.__call__` (diarizen/pipelines/inference.py:137-185): speaker
    counting -> clustering -> inactive speakers to -2 -> reconstruction -> Binarize.  Needs no device, so
    it is checked on the CPU against the oracle's loop-for-loop restatement (tests/test_host.py).
    hook(step_name, artifact): the per-step callback of `SpeakerDiarization.apply`
    (PA/pipelines/speaker_diarization.py:498,572: "speaker_counting", "discrete_diarization").
    soft (optional): the soft multilabel scores f32 [C, L, S] of the same windows — a device tensor (it stays there; with
    `device` given, dzn_speaker_scores aggregates it and only [T, K] comes back) or a host array.  The return value is then
    (Annotation, per-speaker activity scores as a SlidingWindowFeature [T, K]): column k is cluster k = label k of the
    Annotation, T = num_frames (the cropped length) or every frame of the aggregation; the hook sees them as
    "speaker_scores".  The Annotation is the one a call without `soft` returns.
    return_embeddings=True: the clustering's centroids (its third return value, unchanged) go to the hook as "centroids" and
    are appended to the return value as float32 [K, dim], row k = cluster k: (Annotation, embeddings) or
    (Annotation, scores, embeddings)."""
    hook = hook or (lambda *a, **k: None)
    frames = receptive_field(sample_rate)
    hard_decisions = seg.dtype == np.uint8
    # device=...: the two overlap-add aggregations run on the HIP device (postprocess.DevicePost); None = numpy
    post = DevicePost(seg, chunks, frames, device) if device is not None else None
    segf = seg.astype(np.float32) if (post is None or not hard_decisions) else None    # numpy path only
    count = post.speaker_count() if post is not None else speaker_count(segf, chunks, frames)
    hook("speaker_counting", count)
    # the clustering only counts frames of `segmentations`: u8 decisions are counted as bytes (clustering.py)
    hard, _, centroids = clustering(embeddings=emb.astype(np.float64) if emb.dtype != np.float32 else emb,
                            segmentations=seg if hard_decisions else segf, min_clusters=min_speakers,
                            max_clusters=max_speakers)
    embeddings = None
    if return_embeddings:      # (a call without the flag keeps the reference's hook steps, and only those)
        hook("centroids", centroids)
        embeddings = np.asarray(centroids, dtype=np.float32)
    count.data = np.minimum(count.data, max_speakers).astype(np.int8)
    inactive = ~active_speakers(seg) if hard_decisions else np.sum(segf, axis=1) == 0
    hard = np.array(hard, copy=True)
    hard[inactive] = -2
    res = post.reconstruct(hard, count) if post is not None else None
    if res is None and segf is None:
        segf = seg.astype(np.float32)
    discrete, _ = res if res is not None else reconstruct(segf, chunks, hard, count)
    hook("discrete_diarization", discrete)
    result = binarize(discrete, onset=0.5, offset=0.5, uri=sess_name)
    if soft is None:
        return (result, embeddings) if return_embeddings else result
    if post is not None and isinstance(soft, torch.Tensor) and soft.is_cuda:
        scores = post.speaker_scores(hard, soft, num_frames)
    else:
        scores = speaker_scores(soft.cpu().numpy() if isinstance(soft, torch.Tensor) else soft, chunks, frames, hard)
        if num_frames is not None:
            scores.data = np.ascontiguousarray(scores.data[:int(num_frames)])
    hook("speaker_scores", scores)
    return (result, scores, embeddings) if return_embeddings else (result, scores)


def load_hub_config(hub: Path) -> Dict[str, Any]:
    """`<hub>/config.toml` of a DiariZen hub directory ([model], [inference.args], [clustering.args])"""
    with open(Path(hub) / "config.toml", "rb") as f:
        return _toml.load(f)


def resolve_hub(repo_id: str, cache_dir: Optional[str] = None) -> Path:
    """a local hub directory as is, else the HF hub snapshot of `repo_id` (needs network or, with cache_dir, the cache)"""
    if os.path.isdir(repo_id):
        return Path(repo_id).expanduser().absolute()
    from huggingface_hub import snapshot_download
    return Path(snapshot_download(repo_id=repo_id, cache_dir=cache_dir,
                                  local_files_only=cache_dir is not None)).expanduser().absolute()


def open_recording(in_wav, sample_rate: int, lazy: bool = False, resample: str = "host", device=None, channel=0):
    """what `DiariZenPipeline.__call__` accepts (path, BytesIO, bytes or a ProtocolFile mapping with "audio") -> ONE channel
    at `sample_rate`, float32.  channel: an index (default 0, the first channel), "downmix" (audio.downmix: the mean of the
    channels) or an audio.Beamform (array recordings: the channels aligned by GCC-PHAT delays and averaged on `device`; the
    result is an audio.BeamformedSource whatever `lazy` and `resample` say, a file at another rate is beamformed at its own
    rate and resampled on the device, and a sharded run is refused); a mapping's own "channel" key (PA/core/io.py:300-303)
    overrides it, and an index the file does not have is a ValueError.
    lazy=True (sharded runs): a WAV or SPHERE file at that rate is opened as an audio.WavSource / audio.SphereSource, so that every rank decodes only the byte range of its windows (other files need the resampler's
    context and are decoded whole).
    resample="device": a file at ANOTHER rate comes back as an audio.ResampledSource on `device` — nothing is resampled on the
    host, `read_device(start, n)` reads, uploads and resamples (csrc/resample.hip) only the input span of the range, so the
    ranks of a sharded run do that for their own windows only; a WAV or SPHERE file is not decoded here at all (the kernel
    decodes the stored frames, G.711 included, and applies the channel choice).  Files at `sample_rate`
    are returned as with "host", which is the default: the device resampler differs from the host one in the last bits."""
    if resample not in ("host", "device"):
        raise ValueError(f'resample is "host" or "device", not {resample!r}')
    if isinstance(in_wav, Mapping):                    # pyannote ProtocolFile (a Mapping, not a dict)
        if in_wav.get("channel") is not None:          # (None, as in PA/core/io.py:300: no choice of the file's own)
            channel = in_wav["channel"]
        in_wav = in_wav["audio"]
    beamform = channel if isinstance(channel, audio_io.Beamform) else None
    if beamform is None:
        channel = audio_io.check_channel(channel)
    assert isinstance(in_wav, (str, os.PathLike, BytesIO, bytes)), \
        f"input must be either a str, BytesIO or a ProtocolFile; there was {type(in_wav)}"
    if beamform is not None:
        return _open_beamformed(in_wav, sample_rate, device, beamform)
    if (lazy or resample == "device") and isinstance(in_wav, (str, os.PathLike)):
        with open(in_wav, "rb") as f:
            magic = f.read(8)
        opener = audio_io.SphereSource if magic.startswith(b"NIST_1A") else audio_io.WavSource
        try:
            src = opener(in_wav, channel)
            if src.sample_rate == sample_rate:
                if lazy:
                    return src
            elif resample == "device":
                return audio_io.ResampledSource(src, sample_rate, device)
        except ValueError:
            pass                                       # not that container, or a form of it only the whole-file decoders read (or refuse)
    if resample == "device":
        x, sr = audio_io.load_audio(in_wav)
        x0 = audio_io.select_channel(x, channel)       # as first_channel_16k
        return x0 if sr == sample_rate else audio_io.ResampledSource(x0, sample_rate, device, orig_rate=sr)
    return audio_io.first_channel_16k(in_wav, sample_rate, channel)


def _open_beamformed(in_wav, sample_rate: int, device, beamform):
    """open_recording for channel=audio.Beamform(...): an audio.BeamformedSource on `device` over the file's channels.  A WAV
    or SPHERE file on disk is read span by span as stored; anything else is decoded whole by load_audio.  One device only."""
    from . import dist as dz_dist
    if dz_dist.world_size() > 1:
        raise RuntimeError(DiariZenPipeline._ONE_DEVICE % ("channel=Beamform(...)", dz_dist.world_size()))
    src = None
    if isinstance(in_wav, (str, os.PathLike)):
        with open(in_wav, "rb") as f:
            magic = f.read(8)
        opener = audio_io.SphereSource if magic.startswith(b"NIST_1A") else audio_io.WavSource
        try:
            src = opener(in_wav, 0)
        except ValueError:
            src = None                                 # not that container, or a form of it only the whole-file decoders read
    if src is not None:
        return audio_io.BeamformedSource(src, sample_rate, device, beamform)
    x, sr = audio_io.load_audio(in_wav)
    return audio_io.BeamformedSource(x, sample_rate, device, beamform, orig_rate=sr)


def recording_on_device(waveform, device, lo: int = 0, n: Optional[int] = None, zero_extend: bool = False) -> torch.Tensor:
    """samples lo .. lo + n of what open_recording returned (a host array, a lazy source with `.read`, or a source with
    `.read_device`, whose samples are made on the device) as a float32 tensor on `device`; zero_extend: padded with zeros to n
    samples when the recording ends before lo + n (a rank's last window, inference.py:293-299)"""
    if hasattr(waveform, "read_device"):
        n = int(waveform.num_samples) - lo if n is None else n
        wave = waveform.read_device(lo, n)
        if zero_extend and len(wave) < n:
            wave = torch.nn.functional.pad(wave, (0, n - len(wave)))
        return wave
    if hasattr(waveform, "read") and hasattr(waveform, "num_samples"):
        n = int(waveform.num_samples) - lo if n is None else n
        have = waveform.read(lo, n)
    else:
        n = len(waveform) - lo if n is None else n
        have = np.asarray(waveform[lo:lo + n], dtype=np.float32)
    if zero_extend:
        x = np.zeros(n, dtype=np.float32)                      # zero-extended like the last window (inference.py:293-299)
        x[:len(have)] = have
    else:
        x = np.ascontiguousarray(have, dtype=np.float32)
    return torch.from_numpy(x).to(device)


class DiariZenPipeline:
    def __init__(self, diarizen_hub, embedding_model, config_parse: Optional[Dict[str, Any]] = None,
                 rttm_out_dir: Optional[str] = None, *, device: Optional[torch.device] = None,
                 precision: str = "f32h", seg_state: Optional[Mapping[str, torch.Tensor]] = None,
                 emb_state: Optional[Mapping[str, torch.Tensor]] = None,
                 config: Optional[Dict[str, Any]] = None, num_streams: int = 2, resample: str = "host",
                 channel=0):
        """diarizen_hub: directory with config.toml / pytorch_model.bin / plda ; embedding_model: path of
        the WeSpeaker checkpoint.  `seg_state` / `emb_state` / `config` let callers (tests, bench)
        inject in-memory weights instead of files.
        resample: where a recording at another rate than the model's is resampled — "host" (audio.resample, the default) or
        "device" (audio.ResampledSource: the file's samples are uploaded as stored and resampled by csrc/resample.hip, in a
        sharded run every rank only its windows' span; the waveform differs from the host one in its last bits).
        channel: which channel of a recording is diarized — an index (default 0, inference.py:128) or "downmix", the mean of
        the channels (audio.downmix; both sides of a two-channel telephone call), or an audio.Beamform for array recordings
        (GCC-PHAT delay-and-sum on the device, offline only: live sessions and the hub refuse it); a file mapping's "channel"
        key overrides it.
        num_streams (r4): engine handles that consecutive batches of windows alternate over, each on its own HIP stream
        (inference.WindowRunner): independent batches overlap on the device — +2.6 % on the 30-min workload,
        +44 % at 32-window batches (profiles/r4_*), same bits.  Each extra handle costs one more copy of the weights and a
        workspace for `batch_size` windows, so (r5) it is an UPPER bound: the further handles are created lazily, the first time
        a recording has more than one batch, and only while a reserve of HBM stays free (a short recording never pays for
        them); `close()` releases them.  1 = the single-stream engine of r1-r3."""
        hub = Path(diarizen_hub) if diarizen_hub is not None else None
        if config is None:
            config = load_hub_config(hub)
        if config_parse is not None:
            config["inference"]["args"] = config_parse["inference"]["args"]
            config["clustering"]["args"] = config_parse["clustering"]["args"]
        self.config = config
        if resample not in ("host", "device"):
            raise ValueError(f'resample is "host" or "device", not {resample!r}')
        self.resample = resample
        self.channel = channel if isinstance(channel, audio_io.Beamform) else audio_io.check_channel(channel)
        inf, clu = config["inference"]["args"], config["clustering"]["args"]
        if not torch.cuda.is_available():
            raise RuntimeError("DiariZenPipeline (diarizen_amd) needs a HIP device; no CPU fallback")
        self.device = torch.device(device or "cuda:0")

        # ---- plugin boundary: instantiate([model].path, [model].args) + load_state_dict ----
        margs = dict(config["model"]["args"])
        margs.setdefault("precision", precision)
        margs["max_batch"] = int(inf["batch_size"])
        self.segmentation_model: WavLMConformer = instantiate(config["model"]["path"], margs)
        if seg_state is None:
            seg_state = _load_checkpoint(str(hub / "pytorch_model.bin"))
        if emb_state is None:
            emb_state = _load_checkpoint(str(embedding_model))
        emb_state = {k: v for k, v in emb_state.items() if k.startswith("resnet.")}
        self.seg_duration = float(inf["seg_duration"])
        self.segmentation_step = float(inf["segmentation_step"])
        self.batch_size = int(inf["batch_size"])
        self.apply_median_filtering = bool(inf["apply_median_filtering"])
        window = int(self.seg_duration * self.segmentation_model.sample_rate)
        self.engine = Engine(self.segmentation_model.cfg, seg_state, RESNET34, emb_state,
                             max_batch=self.batch_size, max_samples=window, precision=precision,
                             device=self.device)
        # further handles are created by the runner the first time a recording needs more than one batch, and only against a
        # memory reserve (inference.WindowRunner._grow); the factory keeps the host state dicts alive for that
        seg_cfg = self.segmentation_model.cfg

        def _more():
            return Engine(seg_cfg, seg_state, RESNET34, emb_state, max_batch=self.batch_size, max_samples=window,
                          precision=precision, device=self.device)
        self.segmentation_model.load_state_dict(seg_state).bind(self.engine)
        self._embedding = SpeakerEmbedding(engine=self.engine)
        self._runner = WindowRunner(self.engine, self.seg_duration, self.segmentation_step,
                                    self.batch_size, median_size=11 if self.apply_median_filtering else 0,
                                    exclude_overlap=True, engine_factory=_more, max_engines=max(1, int(num_streams)))
        assert self.segmentation_model.specifications.powerset is True

        # ---- clustering (same [clustering.args] keys as the reference) ----
        self.min_speakers, self.max_speakers = clu["min_speakers"], clu["max_speakers"]
        if clu["method"] == "AgglomerativeClustering":
            self.clustering = AgglomerativeClustering(metric="cosine", method="centroid",
                                                      min_cluster_size=clu["min_cluster_size"],
                                                      threshold=clu["ahc_threshold"])
        elif clu["method"] == "VBxClustering":
            self.clustering = VBxClustering(metric="cosine", plda_dir=str(hub / "plda") if hub else "",
                                            lda_dim=clu["lda_dim"], max_iters=clu["max_iters"],
                                            ahc_criterion=clu["ahc_criterion"],
                                            ahc_threshold=clu["ahc_threshold"], Fa=clu["Fa"], Fb=clu["Fb"])
        else:
            raise ValueError(f"Unsupported clustering method: {clu['method']}")
        self.clustering.device = self.device.index if self.device.index is not None else 0   # device linkage (row f1)
        if rttm_out_dir is not None:
            os.makedirs(rttm_out_dir, exist_ok=True)
        self.rttm_out_dir = rttm_out_dir
        self.device_postprocess = True      # speaker counting / reconstruction aggregations on the device (row f2)
        self.timings: Dict[str, float] = {}

    @property
    def extra_engines(self):
        """the further engine handles that exist right now (created lazily by the runner)"""
        return tuple(self._runner.engines[1:])

    def close(self) -> None:
        """release every device allocation of this pipeline (engine handles, their weights and workspaces)"""
        self._runner.close()
        self.engine.close()
        from . import _lib
        _lib.load().dzn_host_workspace_release(self.device.index if self.device.index is not None else 0)   # the host stage's arena

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, repo_id: str, cache_dir: str = None, rttm_out_dir: str = None,
                        **kwargs) -> "DiariZenPipeline":
        """repo_id: HF hub id (needs network/cache, as in the reference) or a local hub directory.
        The embedding checkpoint is `<dir>/wespeaker/pytorch_model.bin` when present locally."""
        hub = resolve_hub(repo_id, cache_dir)
        local = hub / "wespeaker" / "pytorch_model.bin"
        embedding_model = str(local) if os.path.isdir(repo_id) and local.exists() else None
        if embedding_model is None:
            from huggingface_hub import hf_hub_download
            embedding_model = hf_hub_download(repo_id=EMBEDDING_REPO, filename="pytorch_model.bin",
                                              cache_dir=cache_dir, local_files_only=cache_dir is not None)
        return cls(diarizen_hub=hub, embedding_model=embedding_model, rttm_out_dir=rttm_out_dir, **kwargs)

    # ------------------------------------------------------------------ stages
    def chunks_window(self) -> SlidingWindow:
        """SlidingWindow of the (un-aggregated) per-window outputs, PA/core/inference.py:377-381."""
        return SlidingWindow(start=0.0, duration=self.seg_duration,
                             step=self.segmentation_step * self.seg_duration)

    def device_stage(self, waveform, hook=None, with_scores: bool = False):
        """host float32 [N] (or a lazy source with `.num_samples` and `.read(start, n)`, e.g. audio.WavSource, or
        `.read_device(start, n)`, e.g. audio.ResampledSource: its samples are made on the device) ->
        (segmentations u8 [C, L, 4], embeddings f32 [C, 4, 256]) on the host.
        with_scores (one device only): a third element, the soft multilabel scores f32 [C, L, 4], which STAY on the device.
        With torch.distributed initialised, this rank reads / uploads ONLY the samples its contiguous window range touches
        (its slice + one window of halo), runs them, and the per-window results are all-gathered."""
        from . import dist as dz_dist
        r = self._runner
        total = int(waveform.num_samples) if hasattr(waveform, "num_samples") else len(waveform)
        C = r.num_windows(total)
        rng = dz_dist.my_window_range(C)
        if with_scores and dz_dist.world_size() > 1:
            raise RuntimeError(self._ONE_DEVICE % ("device_stage(with_scores=True)", dz_dist.world_size()))
        soft_l = None
        if rng is not None:
            c0, c1 = rng
            lo, n = c0 * r.step, ((c1 - c0 - 1) * r.step + r.window if c1 > c0 else 0)
        else:
            lo, n = 0, total
        if n:
            wave = recording_on_device(waveform, self.device, lo, n, zero_extend=rng is not None)
            res = r.run(wave, with_embeddings=True, hook=hook, with_scores=with_scores)
            seg_l, emb_l, soft_l = res.segmentations, res.embeddings, res.scores
        else:                                                      # more ranks than windows
            S = self.engine.seg.max_speakers_per_chunk
            seg_l = torch.empty((0, r.num_frames, S), device=self.device, dtype=torch.uint8)
            emb_l = torch.empty((0, S, self.engine.emb.embed_dim), device=self.device, dtype=torch.float32)
        # one packed all-gather + ONE device-to-host copy; the copy waits for the CURRENT stream only, which run() joined with the
        # handles' streams - not a device-wide synchronise, which would also wait for the host stage of the previous recording
        # on its own high-priority stream (diarize_many)
        seg, emb = dz_dist.gather_windows(seg_l, emb_l, expected_total=C, to_host=True)
        if with_scores:
            if soft_l is None:
                soft_l = torch.empty((0, r.num_frames, seg_l.shape[2]), device=self.device, dtype=torch.float32)
            return seg.numpy(), emb.numpy(), soft_l
        return seg.numpy(), emb.numpy()

    def host_stage(self, seg: np.ndarray, emb: np.ndarray, sess_name: Optional[str] = None, hook=None, soft=None,
                   num_frames: Optional[int] = None, return_embeddings: bool = False):
        """counting -> clustering -> reconstruction -> Annotation (inference.py:137-185); with `soft` (the device tensor of
        device_stage(with_scores=True)) -> (Annotation, per-speaker activity scores [T, K]), see run_host_stage;
        return_embeddings=True appends the cluster centroids f32 [K, 256]."""
        return run_host_stage(seg, emb, chunks=self.chunks_window(), clustering=self.clustering,
                              min_speakers=self.min_speakers, max_speakers=self.max_speakers,
                              sample_rate=self.segmentation_model.sample_rate, sess_name=sess_name,
                              device=self.device if self.device_postprocess else None, hook=hook, soft=soft,
                              num_frames=num_frames, return_embeddings=return_embeddings)

    _ONE_DEVICE = ("%s runs on one device: the soft scores of a recording sharded over torch.distributed ranks are not "
                   "gathered (world size %d)")

    # ------------------------------------------------------------------ soft / raw segmentation
    def get_segmentations(self, file, soft: bool = False, hook=None) -> SlidingWindowFeature:
        """SpeakerDiarization.get_segmentations(file, hook=None, soft=False) (PA/pipelines/speaker_diarization.py:209-226):
        the per-window output of the segmentation model as a SlidingWindowFeature [C, L, S] float32 on the windows' grid.
        soft=False: the hard decisions BEFORE the median filter (the reference applies its filter in `__call__`,
        diarizen/pipelines/inference.py:131-132, not here); soft=True: Powerset.to_multilabel(soft=True)
        (PA/utils/powerset.py:103-128), written by the classifier kernel.  hook: progress per batch of windows, as
        hook("segmentation", None, file=..., completed=..., total=...)."""
        import functools
        from . import dist as dz_dist
        if dz_dist.world_size() > 1:
            raise RuntimeError(self._ONE_DEVICE % ("get_segmentations", dz_dist.world_size()))
        file = file if isinstance(file, Mapping) else {"audio": file}
        if hook is not None:
            hook = functools.partial(hook, "segmentation", None, file=file)
        x = open_recording(file, self.segmentation_model.sample_rate, resample=self.resample, device=self.device,
                           channel=self.channel)
        # the raw decisions: a runner without the median filter on this pipeline's engine handle(s), as detection._Detection
        raw = WindowRunner(self.engine, self.seg_duration, self.segmentation_step, self.batch_size, median_size=0,
                           exclude_overlap=False, sample_rate=self.segmentation_model.sample_rate,
                           extra_engines=self.extra_engines)
        with torch.cuda.device(self.device):
            res = raw.run(recording_on_device(x, self.device), with_embeddings=False, hook=hook, with_scores=soft)
            data = (res.scores if soft else res.segmentations).cpu().numpy().astype(np.float32, copy=False)
        return SlidingWindowFeature(data, self.chunks_window())

    # ------------------------------------------------------------------ online use
    def stream(self, chunks, sess_name: Optional[str] = None, **kw):
        """windows scheduled as the audio arrives (pinned ring + copy stream): yields (seconds received, provisional
        Annotation) at every refresh and finally (total seconds, final Annotation == __call__ on the whole file).
        See streaming.StreamingSession for the push form (feed / finish).  feed_format=audio.FeedFormat(8000, "ulaw",
        channels=2): the chunks are the source's own bytes (G.711 / PCM frames at 8 .. 48 kHz, any chunk length), decoded,
        channel-selected and resampled on the device; the result is that of the file at that rate with resample="device".
        return_scores=True: (seconds, Annotation, scores) each time — the windows' soft scores stay on the device across feeds
        and the final pair is `__call__(file, return_scores=True)` bit for bit, crop included."""
        from .streaming import stream as _stream
        return _stream(self, chunks, sess_name, **kw)

    def open_live(self, sess_name: Optional[str] = None, delta_new: Optional[float] = None,
                  max_speakers: Optional[int] = None, max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0,
                  slots: int = 4, feed_format=None, scores: bool = False):
        """live diarization with stable labels and a committed prefix: a live.LiveDiarization to `feed(samples)` /
        `finish()`.  delta_new: the centroid distance beyond which a clean local speaker opens a new label (default: the
        config's ahc_threshold); max_speakers: the cap on labels (default: the config's, at most 32); the other keywords size
        the ingest ring (streaming.WaveIngest); feed_format: an audio.FeedFormat when the feeds are the source's own bytes
        (refused here when it cannot be served); scores=True: the session also gives the per-speaker activity scores of
        `__call__(return_scores=True)` live (`committed_scores`, `scores`, `final_scores`) from a device buffer of its windows'
        soft scores, windows x L x S x 4 bytes — about 115 MB at the default max_seconds of 4 h.
        `stream` / StreamingSession stay what they are: provisional re-clusterings
        whose last annotation is the offline result."""
        from .live import LiveDiarization
        return LiveDiarization(self, sess_name, delta_new=delta_new, max_speakers=max_speakers, max_seconds=max_seconds,
                               slot_seconds=slot_seconds, slots=slots, feed_format=feed_format, scores=scores)

    def open_hub(self, max_sessions: int = 64, max_seconds: float = 600.0, slot_bytes: int = 1 << 20, slots: int = 4,
                 array_channels: int = 0, array_rate: Optional[int] = None):
        """many concurrent live sessions, one batched forward per tick: a hub.LiveHub whose `open(name, ...)` takes the
        keywords of open_live but the ingest's and returns a live.LiveDiarization; `feed()` is then host work only and
        `hub.tick()` does the device work of every session at once — one staging upload, one ingest launch, ceil(ready
        windows / batch_size) forwards — with the bits each session would have alone.  max_sessions x max_seconds size ONE
        pooled device buffer (max_sessions x (max_seconds x rate + window) x 4 B: 2.5 GB at the defaults), so max_seconds is
        deliberately far below a solo session's 4 h.  array_channels: the most microphones of an array session
        (`feed_format=FeedFormat(..., channels=C, channel=Beamform(causal=True))`), an integer in [2, 64]; with the default 0
        the hub refuses array feeds and allocates nothing for them.  array_rate: the highest feed rate of an array session
        (default: the model's rate).  All array calls of a tick then share one upload and one dzn_beamform_many."""
        from .hub import LiveHub
        from .live import LiveDiarization
        return LiveHub(self, lambda name, hub, **kw: LiveDiarization(self, name, hub=hub, **kw), max_sessions, max_seconds,
                       slot_bytes, slots, array_channels, array_rate)

    def stream_live(self, chunks, sess_name: Optional[str] = None, **kw):
        """generator form of open_live: yields (seconds received, committed seconds, Annotation) for every feed that has an
        annotation, then the final triple.  Keywords as open_live, and recluster (live.LiveDiarization.finish).  scores=True:
        (seconds, committed seconds, Annotation, scores), scores a SlidingWindowFeature [frames so far, K]."""
        from .live import stream_live as _stream_live
        return _stream_live(self, chunks, sess_name, **kw)

    # ------------------------------------------------------------------ many recordings
    def diarize_many(self, recordings, sess_names=None, overlap: bool = True, return_scores: bool = False,
                     return_embeddings: bool = False):
        """The loop the reference's entry points run over a corpus (diarizen/pipelines/inference.py:365-368: `for audio_file in
        audio_f: diarizen_pipeline(audio_file, sess_name=...)`; recipes/diar_ssl/infer_avg.py:334-338), as a generator of
        (sess_name, Annotation) in input order, with the SAME result per recording as `__call__`.
        overlap=True (r5): a software pipeline over the recordings — recording i+1 is decoded by a loader thread and the host
        stage of recording i-1 (counting, AHC / VBx, assignment, reconstruction, RTTM) runs in a worker thread while this thread
        uploads recording i and runs its device stage (at most two decoded recordings are alive at a time).  The host stage's device work has its own high-priority stream and workspace (csrc/linkage.hip,
        postprocess.DevicePost), so neither side queues behind the other; on the 30-min workload the host stage is 70 ms
        against 1.04 s of device stage, i.e. the corpus rate becomes the device rate.  At most one finished device stage
        waits for the worker (its seg / emb arrays: a few MB per hour of audio).  With torch.distributed initialised every
        rank calls this with the same list; only rank 0 yields Annotations (the others yield None), as in `__call__`.
        return_scores=True (one device only): (sess_name, Annotation, scores) with the scores of `__call__(return_scores=True)`;
        the soft scores of a recording stay on the device and travel with its pending host stage.
        return_embeddings=True: the cluster centroids f32 [K, 256] of `__call__(return_embeddings=True)` are appended to every
        tuple, after the scores when both are asked for (ranks other than 0: None, as the Annotation)."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from . import dist as dz_dist
        recordings = list(recordings)
        if sess_names is None:
            sess_names = [Path(r).stem.split('.')[0] if isinstance(r, (str, os.PathLike)) else None for r in recordings]
        sess_names = list(sess_names)
        if len(sess_names) != len(recordings):
            raise ValueError("diarize_many: one session name per recording")
        if return_scores and dz_dist.world_size() > 1:
            raise RuntimeError(self._ONE_DEVICE % ("diarize_many(return_scores=True)", dz_dist.world_size()))
        if not overlap:
            for rec, name in zip(recordings, sess_names):
                if return_scores or return_embeddings:
                    yield (name, *self(rec, sess_name=name, return_scores=return_scores, return_embeddings=return_embeddings))
                else:
                    yield (name, self(rec, sess_name=name))
            return
        rank0 = dz_dist.rank() == 0

        want = {"return_embeddings": True} if return_embeddings else {}      # (a call without the flag is the parent's call)

        def host(seg, emb, name, soft=None, n=0):
            t = time.perf_counter()
            if soft is None:
                res = self.host_stage(seg, emb, name, **want)
                ann = res[0] if return_embeddings else res
            else:                                        # the crop rule of __call__
                r = self._runner
                grid, _, T = _frame_grid(seg.shape[0], seg.shape[1], self.chunks_window(),
                                         receptive_field(self.segmentation_model.sample_rate))
                if window_plan(n, r.window, r.step)[1]:
                    T = crop_end(T, grid, n / self.segmentation_model.sample_rate)
                with torch.cuda.device(self.device):
                    res = self.host_stage(seg, emb, name, soft=soft, num_frames=T, **want)
                ann = res[0]
            if self.rttm_out_dir is not None:
                assert name is not None
                with open(os.path.join(self.rttm_out_dir, name + ".rttm"), "w") as f:
                    f.write(ann.to_rttm())
            return res, time.perf_counter() - t

        def load(rec):
            t = time.perf_counter()
            w = self._open(rec)
            return w, time.perf_counter() - t

        self.corpus_timings = []
        pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dzn-host-stage")
        loader = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dzn-decode")      # recording i+1 is decoded beside device stage i
        pending = None                                   # (future, name, load_s, device_s, audio_s, what a rank without one yields)
        blank = (None,) * (1 + int(return_scores) + int(return_embeddings)) if return_embeddings else None
        try:
            nxt = loader.submit(load, recordings[0]) if recordings else None
            for i, name in enumerate(sess_names):
                waveform, load_s = nxt.result()
                nxt = loader.submit(load, recordings[i + 1]) if i + 1 < len(recordings) else None
                n = int(waveform.num_samples) if hasattr(waveform, "num_samples") else len(waveform)
                t1 = time.perf_counter()
                if return_scores:
                    seg, emb, soft = self.device_stage(waveform, with_scores=True)
                else:
                    (seg, emb), soft = self.device_stage(waveform), None
                t2 = time.perf_counter()
                del waveform
                if pending is not None:                  # recording i-1's host stage ran beside this device stage
                    yield self._collect(pending)
                fut = pool.submit(host, seg, emb, name, soft, n) if rank0 else None
                del soft
                pending = (fut, name, load_s, t2 - t1, n / self.segmentation_model.sample_rate, blank)
            if pending is not None:
                yield self._collect(pending)
        finally:
            loader.shutdown(wait=True, cancel_futures=True)
            pool.shutdown(wait=True)

    def _collect(self, pending):
        fut, name, load_s, device_s, audio_s, blank = pending
        res, host_s = fut.result() if fut is not None else (blank, 0.0)
        self.timings = {"load_s": load_s, "device_s": device_s, "host_s": host_s, "audio_s": audio_s}
        self.corpus_timings.append(dict(self.timings, sess_name=name))
        return (name, *res) if isinstance(res, tuple) else (name, res)

    def link_many(self, recordings, threshold: float, sess_names=None, fmt: str = "spk{:04d}", backend: str = "auto"):
        """Diarize a corpus and link its speakers across recordings (linking.SpeakerLinker; no reference counterpart):
        `diarize_many(return_embeddings=True)`, every recording's centroids into ONE linker, one complete-linkage clustering
        under the rule that two labels of one recording are different people, cut at `threshold` — a cosine distance in (0, 2],
        required, no default (nothing here can calibrate one).  -> ({sess_name: Annotation whose labels are the corpus-wide
        names fmt.format(identity)}, linking.SpeakerLinks).  Session names must be distinct.  With rttm_out_dir set the
        per-recording RTTM files are rewritten with the global names after linking.  In a sharded run rank 0 has the result;
        other ranks run the device stages and return ({}, None)."""
        from . import dist as dz_dist
        from .linking import SpeakerLinker
        SpeakerLinker(threshold, backend=backend)            # a bad threshold or backend is refused before any device work
        annotations, voiceprints = {}, {}
        for name, annotation, centroids in self.diarize_many(recordings, sess_names=sess_names, return_embeddings=True):
            if annotation is None:                           # a rank other than 0
                continue
            if name is None:
                raise ValueError("link_many: every recording needs a session name")
            if name in annotations:
                raise ValueError(f"link_many: session name {name!r} twice")
            annotations[name], voiceprints[name] = annotation, np.asarray(centroids, dtype=np.float32)
        if dz_dist.rank() != 0:
            return {}, None
        dims = [v.shape[1] for v in voiceprints.values() if v.ndim == 2 and v.shape[0]]
        linker = SpeakerLinker(threshold, dim=dims[0] if dims else 256, device=self.device, backend=backend)
        for name, v in voiceprints.items():
            linker.add(name, v)
        links = linker.link()
        out = {name: links.relabel(name, ann, fmt) for name, ann in annotations.items()}
        if self.rttm_out_dir is not None:
            for name, ann in out.items():
                with open(os.path.join(self.rttm_out_dir, name + ".rttm"), "w") as f:
                    f.write(ann.to_rttm())
        return out, links

    def link_into(self, registry, recordings, sess_names=None, fmt: str = "spk{:04d}"):
        """Diarize a corpus and link every recording into a growing registry AS IT FINISHES (registry.SpeakerRegistry; no
        reference counterpart): a generator over `diarize_many(return_embeddings=True)` of (sess_name, Annotation whose labels
        are the corpus-wide names fmt.format(identity), {label: identity}).  Unlike `link_many` nothing waits for the end of the
        corpus, and the registry may already hold earlier corpora: identity numbers never change.  Session names must be given
        and new to the registry.  With rttm_out_dir set each recording's RTTM file is rewritten with the global names.  In a
        sharded run rank 0 yields; other ranks run the device stages and yield nothing."""
        from .identification import relabel
        if sess_names is not None:                           # refused before any device work
            sess_names = list(sess_names)
            if any(name is None for name in sess_names):
                raise ValueError("link_into: every recording needs a session name")
            if len(set(sess_names)) != len(sess_names):
                raise ValueError("link_into: a session name twice")
            known = [name for name in sess_names if name in registry]
            if known:
                raise ValueError(f"link_into: the registry already holds {known!r}")
        for name, annotation, centroids in self.diarize_many(recordings, sess_names=sess_names, return_embeddings=True):
            if annotation is None:                           # a rank other than 0
                continue
            if name is None:
                raise ValueError("link_into: every recording needs a session name")
            ids = registry.add(name, np.asarray(centroids, dtype=np.float32))
            out = relabel(annotation, {label: fmt.format(i) for label, i in ids.items()})
            if self.rttm_out_dir is not None:
                with open(os.path.join(self.rttm_out_dir, name + ".rttm"), "w") as f:
                    f.write(out.to_rttm())
            yield name, out, ids

    def _open(self, in_wav):
        """decode (or, in a sharded run, lazily open) one recording: the first lines of `__call__`"""
        from . import dist as dz_dist
        return open_recording(in_wav, self.segmentation_model.sample_rate, lazy=dz_dist.world_size() > 1,
                              resample=self.resample, device=self.device, channel=self.channel)

    # ------------------------------------------------------------------ __call__
    def __call__(self, in_wav, sess_name: Optional[str] = None, hook=None, return_scores: bool = False,
                 return_embeddings: bool = False):
        """`hook` (optional, not in the reference's DiariZenPipeline signature but in the pyannote pipeline it
        derives from): hook(step_name, step_artifact, file=..., total=..., completed=...) as
        PA/pipelines/utils/hook.py:36-224 expects (ProgressHook / ArtifactHook / TimingHook work unchanged).
        Steps: "segmentation" (progress per batch of windows, then the SlidingWindowFeature), "speaker_counting",
        "embeddings" (the [C, S, 256] array — computed in the same device pass as the segmentation, so it has no
        progress of its own), "discrete_diarization".
        return_scores=True: -> (Annotation, scores), scores a SlidingWindowFeature f32 [T, K] of per-speaker activity scores on
        the frame grid of the discrete diarization: the soft multilabel scores of every window (Powerset.to_multilabel(
        soft=True)) mapped to the clusters as reconstruct does and aggregated with Inference.aggregate(hamming=True,
        missing=0.0).  Column k is cluster k, the integer label k of the Annotation (K = max(hard_clusters) + 1: a cluster
        that never wins a frame keeps its column); T is cropped at the end of the audio when the last window was zero-padded.
        The Annotation and the RTTM file are those of a call without the flag; the hook also sees "speaker_scores".
        return_embeddings=True (SpeakerDiarization.apply(return_embeddings=True), PA/pipelines/speaker_diarization.py:433,
        612-636): -> (Annotation, embeddings), or (Annotation, scores, embeddings) together with return_scores.  embeddings is
        float32 [K, 256], the clustering's centroids: row k is cluster k, the integer label k of the Annotation — the convention
        of the return_scores columns, a cluster that wins no frame keeps its row.  One deviation from pyannote: it re-orders
        the rows by `labels()`; our labels already are the cluster indices, so nothing is re-ordered.  The Annotation and the
        RTTM file are those of a call without the flag; in a sharded run rank 0 has the centroids (other ranks: None)."""
        import functools
        import time
        file = in_wav if isinstance(in_wav, Mapping) else {"audio": in_wav}
        if hook is not None:
            hook = functools.partial(hook, file=file)       # Pipeline.setup_hook (PA/core/pipeline.py:267-271)
        t0 = time.perf_counter()
        from . import dist as dz_dist
        if return_scores and dz_dist.world_size() > 1:
            raise RuntimeError(self._ONE_DEVICE % ("return_scores=True", dz_dist.world_size()))
        waveform = self._open(in_wav)                      # (a mapping's "channel" key is read there)
        num_samples = int(waveform.num_samples) if hasattr(waveform, "num_samples") else len(waveform)
        t1 = time.perf_counter()
        soft = None
        seg_hook = functools.partial(hook, "segmentation", None) if hook is not None else None
        if return_scores:
            seg, emb, soft = self.device_stage(waveform, hook=seg_hook, with_scores=True)
        else:
            seg, emb = self.device_stage(waveform, hook=seg_hook)
        if hook is not None:
            hook("segmentation", SlidingWindowFeature(seg, self.chunks_window()))
            hook("embeddings", emb)
        t2 = time.perf_counter()
        result = scores = embeddings = None
        if dz_dist.rank() == 0:
            if return_scores:
                r = self._runner
                grid, _, T = _frame_grid(seg.shape[0], seg.shape[1], self.chunks_window(),
                                         receptive_field(self.segmentation_model.sample_rate))
                if window_plan(num_samples, r.window, r.step)[1]:
                    T = crop_end(T, grid, num_samples / self.segmentation_model.sample_rate)   # PA/core/inference.py:400-403
                out = self.host_stage(seg, emb, sess_name, hook=hook, soft=soft, num_frames=T,
                                      return_embeddings=return_embeddings)
                result, scores = out[0], out[1]
                embeddings = out[2] if return_embeddings else None
            elif return_embeddings:
                result, embeddings = self.host_stage(seg, emb, sess_name, hook=hook, return_embeddings=True)
            else:
                result = self.host_stage(seg, emb, sess_name, hook=hook)
            if self.rttm_out_dir is not None:
                assert sess_name is not None
                with open(os.path.join(self.rttm_out_dir, sess_name + ".rttm"), "w") as f:
                    f.write(result.to_rttm())
        t3 = time.perf_counter()
        self.streams_in_use = len(self._runner.engines)       # <= num_streams (WindowRunner.grow_declined says why when fewer)
        self.timings = {"load_s": t1 - t0, "device_s": t2 - t1, "host_s": t3 - t2,
                        "audio_s": num_samples / self.segmentation_model.sample_rate}
        if return_embeddings:
            return (result, scores, embeddings) if return_scores else (result, embeddings)
        return (result, scores) if return_scores else result

    def resegment(self, file, diarization=None, hook=None, **params):
        """refine a given diarization of `file` with this pipeline's segmentation model: resegmentation.Resegmentation over
        this pipeline's engine (no second copy of the weights), instantiated with **params (warm_up, min_duration_on,
        min_duration_off).  -> (Annotation with integer labels, the hypothesis's labels sorted: column k is labels[k])"""
        from .resegmentation import Resegmentation
        reseg = Resegmentation(self, rttm_out_dir=self.rttm_out_dir).instantiate(params)
        try:
            return reseg(file, diarization=diarization, hook=hook), reseg.labels
        finally:
            reseg.close()               # the borrowed engine stays open

    def voiceprint(self, in_wav, sess_name: Optional[str] = None) -> np.ndarray:
        """the enrolment call: float32 [256], the centroid of the label with the largest total duration in the recording (ties:
        the smaller label).  ValueError when the recording has no speech."""
        annotation, embeddings = self(in_wav, sess_name=sess_name, return_embeddings=True)
        duration: Dict[int, float] = {}
        for segment, _, label in annotation.itertracks(yield_label=True):
            duration[int(label)] = duration.get(int(label), 0.0) + segment.duration
        if not duration:
            raise ValueError("voiceprint: the recording has no speech")
        best = min(duration, key=lambda k: (-duration[k], k))
        return np.array(embeddings[best], dtype=np.float32, copy=True)
