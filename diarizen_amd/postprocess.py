"""Host post-processing between the device stages and the RTTM: overlap-add aggregation,
instantaneous speaker count, reconstruction of the global diarization and binarisation.

Restates, with numpy vector ops instead of per-frame Python loops ("f2" row of SURVEY.md §8f):
  * Inference.aggregate                      PA/core/inference.py:544-666
  * SpeakerDiarizationMixin.speaker_count    PA/pipelines/utils/diarization.py:121-157
  * SpeakerDiarizationMixin.to_diarization   PA/pipelines/utils/diarization.py:192-239
  * SpeakerDiarization.reconstruct           PA/pipelines/speaker_diarization.py:377-425
  * Binarize.__call__ (onset = offset = 0.5) PA/utils/signal.py:254-317
  * Powerset.to_multilabel(soft=True)        PA/utils/powerset.py:103-128   (soft_multilabel, speaker_scores)
The frame grid is SlidingWindow(start = chunks.start, duration = 0.025, step = 0.02): the
receptive-field START is discarded by aggregate() (inference.py:577-581) — kept as is.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import _lib
from .core import HAVE_PYANNOTE_CORE, Annotation, Segment, SlidingWindow, SlidingWindowFeature


def receptive_field(sample_rate: int = 16000) -> SlidingWindow:
    """Model._receptive_field (PA/core/model.py:180-195) for the 7-conv WavLM extractor
    (k = 10,3,3,3,3,2,2 ; s = 5,2,2,2,2,2,2): size 400 samples, step 320, centre of frame 0 at
    sample 79 -> start = (79 - 199.5)/sr = -0.00753125 s."""
    k = [10, 3, 3, 3, 3, 2, 2]
    s = [5, 2, 2, 2, 2, 2, 2]

    def size(n):
        for kk, ss in zip(reversed(k), reversed(s)):
            n = 1 + (kk - 1) + (n - 1) * ss
        return n

    def center(frame):       # PA/utils/receptive_field.py: frame*stride + (k-1)//2, innermost conv last
        c = int(frame)
        for kk, ss in zip(reversed(k), reversed(s)):
            c = c * ss + (kk - 1) // 2
        return c

    sz = size(1)
    st = size(2) - sz
    start = center(0) - (sz - 1) / 2
    return SlidingWindow(start=start / sample_rate, duration=sz / sample_rate, step=st / sample_rate)


def aggregate(scores: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, *, hamming: bool = False,
              missing: float = np.nan, skip_average: bool = False, epsilon: float = 1e-12
              ) -> SlidingWindowFeature:
    """scores [C, L, K] (NaN = missing) with window c covering [chunks.start + c*step, +duration).
    warm_up is (0, 0) on this path (diarizen/pipelines/inference.py:138-142)."""
    C, L, K = scores.shape
    frames = SlidingWindow(start=chunks.start, duration=frames.duration, step=frames.step)
    mask = (~np.isnan(scores)).astype(np.float32)
    data = np.nan_to_num(scores, nan=0.0).astype(np.float32)
    win = (np.hamming(L) if hamming else np.ones(L)).reshape(-1, 1).astype(np.float64)
    num_frames = frames.closest_frame(chunks.start + chunks.duration + (C - 1) * chunks.step
                                      + 0.5 * frames.duration) + 1
    out = np.zeros((num_frames, K), dtype=np.float32)
    cnt = np.zeros((num_frames, K), dtype=np.float32)
    seen = np.zeros((num_frames, K), dtype=np.float32)
    for c in range(C):
        s0 = frames.closest_frame(chunks.start + c * chunks.step + 0.5 * frames.duration)
        out[s0:s0 + L] += data[c] * mask[c] * win
        cnt[s0:s0 + L] += mask[c] * win
        np.maximum(seen[s0:s0 + L], mask[c], out=seen[s0:s0 + L])
    avg = out if skip_average else out / np.maximum(cnt, epsilon)
    avg[seen == 0.0] = missing
    return SlidingWindowFeature(avg, frames)


def speaker_count(segmentations: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow
                  ) -> SlidingWindowFeature:
    """[C, L, S] {0,1} -> (num_frames, 1) uint8 instantaneous speaker count."""
    tot = np.sum(segmentations.astype(np.float32), axis=-1, keepdims=True)
    count = aggregate(tot, chunks, frames, hamming=False, missing=0.0, skip_average=False)
    count.data = np.rint(count.data).astype(np.uint8)
    return count


def to_diarization(clustered: np.ndarray, chunks: SlidingWindow, count: SlidingWindowFeature
                   ) -> Tuple[SlidingWindowFeature, SlidingWindowFeature]:
    act = aggregate(clustered, chunks, count.sliding_window, hamming=False, missing=0.0,
                    skip_average=True)
    return _select_top_count(act, count)


def reconstruct(segmentations: np.ndarray, chunks: SlidingWindow, hard_clusters: np.ndarray,
                count: SlidingWindowFeature) -> Tuple[SlidingWindowFeature, SlidingWindowFeature]:
    """segmentations [C, L, S], hard_clusters [C, S] (-2 = inactive) -> discrete diarization."""
    C, L, S = segmentations.shape
    K = int(np.max(hard_clusters)) + 1 if hard_clusters.size else 0
    K = max(K, 0)
    clustered = np.full((C, L, K), np.nan, dtype=np.float64)
    seg = segmentations.astype(np.float64)
    for k in range(K):
        sel = hard_clusters == k                                   # [C, S]
        has = sel.any(axis=1)
        if not has.any():
            continue
        vals = np.where(sel[:, None, :], seg, -np.inf).max(axis=2)  # max over local speakers -> [C, L]
        clustered[has, :, k] = vals[has]
    return to_diarization(clustered, chunks, count)


# ----------------------------------------------------------------------------- per-speaker activity scores
def soft_multilabel(logp: np.ndarray, mapping: np.ndarray) -> np.ndarray:
    """Powerset.to_multilabel(powerset, soft=True) (PA/utils/powerset.py:120-128): exp(logp) @ mapping in float32.
    logp [..., n_classes] log-probabilities, mapping [n_classes, S] {0,1} -> [..., S]."""
    return np.matmul(np.exp(np.asarray(logp, dtype=np.float32)), np.asarray(mapping, dtype=np.float32))


def aggregation_windows(L: int, duration: float, warm_up=(0.0, 0.0), epsilon: float = 1e-12):
    """the two float64 [L] factors of Inference.aggregate(hamming=True, warm_up) (PA/core/inference.py:586-607), kept apart:
    the reference multiplies (score * hamming) * warm_up, and for scores that are not 0 / 1 a pre-multiplied table does not
    round the same way"""
    wu = np.ones(L, dtype=np.float64)
    left = round(warm_up[0] / duration * L)
    wu[:left] = epsilon
    right = round(warm_up[1] / duration * L)
    wu[L - right:] = epsilon
    return np.ascontiguousarray(np.hamming(L), dtype=np.float64), wu


def clustered_scores(soft: np.ndarray, hard_clusters: np.ndarray) -> np.ndarray:
    """the clustered segmentations of SpeakerDiarization.reconstruct (PA/pipelines/speaker_diarization.py:400-423) on soft
    scores: float64 [C, L, K], K = max(hard) + 1, clustered[c, :, k] = max over the local speakers s of window c with
    hard[c, s] == k, NaN when there is none (hard < 0 = inactive is skipped)"""
    soft = np.asarray(soft, dtype=np.float32)
    hard_clusters = np.asarray(hard_clusters)
    C, L, S = soft.shape
    K = max(int(np.max(hard_clusters)) + 1, 0) if hard_clusters.size else 0
    clustered = np.full((C, L, K), np.nan, dtype=np.float64)
    for k in range(K):
        sel = hard_clusters == k                                    # [C, S]
        has = sel.any(axis=1)
        if not has.any():
            continue
        vals = np.where(sel[:, None, :], soft, np.float32(-np.inf)).max(axis=2)     # [C, L] float32 (NaN propagates like np.max)
        clustered[has, :, k] = vals[has]
    return clustered


def speaker_scores(soft: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, hard_clusters: np.ndarray,
                   warm_up=(0.0, 0.0), epsilon: float = 1e-12) -> SlidingWindowFeature:
    """soft f32 [C, L, S] (soft multilabel scores of every window), hard_clusters [C, S] (-2 = inactive) -> per-speaker
    activity scores f32 [T, K]: reconstruct's clustered scores through Inference.aggregate(hamming=True, missing=0.0,
    skip_average=False, warm_up) (PA/core/inference.py:544-666), with its arithmetic: float64 operands added window after
    window into float32 arrays, (score * mask) * hamming * warm_up in that order.  Needs no device; dzn_speaker_scores
    (csrc/post.hip) is checked against it bit for bit."""
    clustered = clustered_scores(soft, hard_clusters)
    C, L, K = clustered.shape
    grid, starts, T = _frame_grid(C, L, chunks, frames)
    mask = 1 - np.isnan(clustered)                                  # int64, as in the reference
    data = np.nan_to_num(clustered, copy=True, nan=0.0)
    ham, wu = (w.reshape(-1, 1) for w in aggregation_windows(L, chunks.duration, warm_up, epsilon))
    out = np.zeros((T, K), dtype=np.float32)
    cnt = np.zeros((T, K), dtype=np.float32)
    seen = np.zeros((T, K), dtype=np.float32)
    for c in range(C):
        s0 = int(starts[c])
        out[s0:s0 + L] += data[c] * mask[c] * ham * wu
        cnt[s0:s0 + L] += mask[c] * ham * wu
        np.maximum(seen[s0:s0 + L], mask[c], out=seen[s0:s0 + L])
    avg = out / np.maximum(cnt, np.float32(epsilon))
    avg[seen == 0.0] = 0.0
    return SlidingWindowFeature(avg, grid)


def speaker_scores_range(soft: np.ndarray, hard_clusters: np.ndarray, starts: np.ndarray, t0: int, t1: int, K: int,
                         duration: float, warm_up=(0.0, 0.0), epsilon: float = 1e-12) -> np.ndarray:
    """speaker_scores for a FIXED number of columns K and the frames [t0, t1) only — the numpy restatement of the scores of
    dzn_diarize_range_scores (needs no device; the kernel is checked against it bit for bit): soft f32 [C, L, S], hard_clusters
    [C, S] (labels < 0 or >= K match no column), starts int [C] the windows' start frames, duration the windows' length in
    seconds (the warm-up table's unit) -> f32 [t1 - t0, K], row t - t0.  A frame's score sees the windows that cover it in
    ascending order with speaker_scores' arithmetic, so the concatenation over a partition of [0, T) is the [0, T) result, and
    columns [0, max(hard) + 1) of a call with a larger K are those of speaker_scores; a column no window holds is zeros."""
    soft = np.asarray(soft, dtype=np.float32)
    hard_clusters = np.asarray(hard_clusters)
    C, L, S = soft.shape
    t0, t1, K = int(t0), int(t1), int(K)
    n = max(t1 - t0, 0)
    ham, wu = (w.reshape(-1, 1) for w in aggregation_windows(L, duration, warm_up, epsilon))
    out = np.zeros((n, K), dtype=np.float32)
    cnt = np.zeros((n, K), dtype=np.float32)
    seen = np.zeros((n, K), dtype=np.float32)
    for c in range(C):
        s0 = int(starts[c])
        a, b = max(s0, t0), min(s0 + L, t1)                         # the frames of window c inside the range
        if a >= b:
            continue
        clustered = np.full((b - a, K), np.nan, dtype=np.float64)   # float64 holding float32 values, as in the reference
        for k in range(K):
            sel = hard_clusters[c] == k
            if sel.any():
                clustered[:, k] = soft[c, a - s0:b - s0][:, sel].max(axis=1)      # float32 max; a NaN propagates
        mask = 1 - np.isnan(clustered)
        data = np.nan_to_num(clustered, copy=True, nan=0.0)
        h, w = ham[a - s0:b - s0], wu[a - s0:b - s0]
        out[a - t0:b - t0] += data * mask * h * w
        cnt[a - t0:b - t0] += mask * h * w
        np.maximum(seen[a - t0:b - t0], mask, out=seen[a - t0:b - t0])
    avg = out / np.maximum(cnt, np.float32(epsilon))
    avg[seen == 0.0] = 0.0
    return avg


# ----------------------------------------------------------------------------- device versions (row f2)
def _aggregate_grid(chunks: SlidingWindow, frames: SlidingWindow) -> SlidingWindow:
    """the frame grid of aggregate(): the receptive field's duration and step from the chunks' start"""
    return SlidingWindow(start=chunks.start, duration=frames.duration, step=frames.step)


def committed_frames(num_windows: int, chunks: SlidingWindow, frames: SlidingWindow, grid: Optional[SlidingWindow] = None) -> int:
    """the start frame of window index `num_windows` — the reference's float64 closest_frame arithmetic
    (PA/core/inference.py:611-620): with windows 0 .. num_windows - 1 computed, every frame before it is covered by computed
    windows only, so its aggregated score — and the hysteresis up to it — is final; the frame itself is the first that the
    next window changes (streaming.CommittedStream).  grid: aggregate's grid when the caller has it already."""
    grid = _aggregate_grid(chunks, frames) if grid is None else grid
    return int(grid.closest_frame(chunks.start + num_windows * chunks.step + 0.5 * grid.duration))


def covered_frames(num_windows: int, chunks: SlidingWindow, frames: SlidingWindow, grid: Optional[SlidingWindow] = None) -> int:
    """number of frames Inference.aggregate gives for `num_windows` windows (PA/core/inference.py:577-581, 645)"""
    grid = _aggregate_grid(chunks, frames) if grid is None else grid
    return int(grid.closest_frame(chunks.start + chunks.duration + (num_windows - 1) * chunks.step + 0.5 * grid.duration) + 1)


def _frame_grid(C: int, L: int, chunks: SlidingWindow, frames: SlidingWindow):
    """(frame grid of aggregate(), start frame of every window, number of output frames): the arithmetic stays on the host"""
    grid = _aggregate_grid(chunks, frames)
    starts = np.array([committed_frames(c, chunks, frames, grid) for c in range(C)], dtype=np.int32)
    return grid, starts, covered_frames(C, chunks, frames, grid)


def _call(name: str, *args) -> None:
    """one C-ABI launch (include/dzn.h) on the current stream of the operands' device (that of the first, a tensor): numbers
    go over as they are, None as a null pointer, everything else is a device tensor and goes over as its address; the stream
    handle is appended and the status goes through _lib.check"""
    import torch
    argv = [a if a is None or isinstance(a, (int, float)) else a.data_ptr() for a in args]
    _lib.check(getattr(_lib.load(), name)(*argv, torch.cuda.current_stream(args[0].device).cuda_stream), None, name)


_HOST_STREAMS = {}


def _host_stream(device):
    """one high-priority non-blocking stream per device for the host stage's aggregations (the C side keeps its own for the
    linkage / cdist calls, csrc/linkage.hip)"""
    import torch
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _HOST_STREAMS.get(key)
    if st is None:
        st = _HOST_STREAMS[key] = torch.cuda.Stream(device=device, priority=-1)
    return st


class DevicePost:
    """speaker_count / reconstruct with their overlap-add aggregations on the HIP device (dzn_speaker_count,
    dzn_cluster_activations: integer atomics over the u8 decisions).  The decisions are uploaded once (3.6 MB per
    30 min); the top-`count` selection per frame keeps the reference's numpy call on the downloaded activations."""

    def __init__(self, segmentations: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, device):
        import torch
        self.torch = torch
        _lib.load()                                                 # a missing library is an error here, not at the first launch
        self.device = torch.device(device)
        seg = np.ascontiguousarray(segmentations)
        if seg.dtype != np.uint8:
            if not np.array_equal(seg, seg.astype(np.uint8)):
                raise ValueError("DevicePost needs hard {0,1} decisions")
            seg = seg.astype(np.uint8)
        self.C, self.L, self.S = seg.shape
        self.chunks, self.frames = chunks, frames
        self.grid, starts, self.T = _frame_grid(self.C, self.L, chunks, frames)
        # (r5) the host stage's own stream: it may run in a second thread while the engine executes the next recording's
        # device stage (pipeline.diarize_many), and work queued on the default stream would wait behind the engine's
        self.stream = _host_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self.seg = torch.from_numpy(seg).to(self.device)
            self.starts = torch.from_numpy(starts).to(self.device)

    @classmethod
    def from_device(cls, seg_t, chunks: SlidingWindow, frames: SlidingWindow) -> "DevicePost":
        """the same object over decisions u8 [C, L, S] that are already on the device (no download, no second upload): the
        host stage's stream first waits for the current stream, where they were produced"""
        import torch
        _lib.load()
        assert seg_t.is_cuda and seg_t.dtype == torch.uint8 and seg_t.is_contiguous() and seg_t.dim() == 3
        self = cls.__new__(cls)
        self.torch, self.device = torch, seg_t.device
        self.C, self.L, self.S = (int(d) for d in seg_t.shape)
        self.chunks, self.frames = chunks, frames
        self.grid, starts, self.T = _frame_grid(self.C, self.L, chunks, frames)
        self.stream = _host_stream(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            seg_t.record_stream(self.stream)
            self.seg = seg_t
            self.starts = torch.from_numpy(starts).to(self.device)
        return self

    def speaker_count(self) -> SlidingWindowFeature:
        torch = self.torch
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            work = torch.empty(2 * self.T, device=self.device, dtype=torch.int32)
            out = torch.empty(self.T, device=self.device, dtype=torch.uint8)
            _call("dzn_speaker_count", self.seg, self.C, self.L, self.S, self.starts, self.T, work, out)
            return SlidingWindowFeature(out.cpu().numpy().reshape(-1, 1), self.grid)

    def reconstruct(self, hard_clusters: np.ndarray, count: SlidingWindowFeature, num_clusters: Optional[int] = None):
        """num_clusters: the number of activation columns when the caller fixes it (resegmentation: one column per speaker of
        the padded matching, also those no window was assigned to); default max(hard_clusters) + 1"""
        torch = self.torch
        K = int(np.max(hard_clusters)) + 1 if hard_clusters.size else 0
        if num_clusters is not None:
            K = max(K, int(num_clusters))
        if K < 1 or K > 32:
            return None                                     # caller falls back to the numpy path
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            hard = torch.from_numpy(np.ascontiguousarray(hard_clusters, dtype=np.int8)).to(self.device)
            act = torch.empty((self.T, K), device=self.device, dtype=torch.int32)
            _call("dzn_cluster_activations", self.seg, hard, self.C, self.L, self.S, self.starts, self.T, K, act)
            a = act.cpu().numpy().astype(np.float32)
        return _select_top_count(SlidingWindowFeature(a, count.sliding_window), count)

    def speaker_scores(self, hard_clusters: np.ndarray, soft_device, num_frames: Optional[int] = None,
                       warm_up=(0.0, 0.0)) -> SlidingWindowFeature:
        """per-speaker activity scores f32 [T, K] (dzn_speaker_scores) from the soft scores f32 [C, L, S] that are still on
        the device; T = num_frames (the cropped length) or the full aggregate length.  Only [T, K] comes back.  K > 32 takes
        the numpy function, as reconstruct does."""
        torch = self.torch
        T = self.T if num_frames is None else int(num_frames)
        K = max(int(np.max(hard_clusters)) + 1, 0) if hard_clusters.size else 0
        if K < 1 or T < 1:
            return SlidingWindowFeature(np.zeros((max(T, 0), K), dtype=np.float32), self.grid)
        if K > 32:
            host = speaker_scores(soft_device.cpu().numpy(), self.chunks, self.frames, hard_clusters, warm_up)
            return SlidingWindowFeature(np.ascontiguousarray(host.data[:T]), self.grid)
        assert soft_device.is_cuda and soft_device.dtype == torch.float32 and soft_device.is_contiguous()
        assert tuple(soft_device.shape) == (self.C, self.L, self.S)
        ham, wu = aggregation_windows(self.L, self.chunks.duration, warm_up)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))     # the soft scores were produced there
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            soft_device.record_stream(self.stream)
            hard = torch.from_numpy(np.ascontiguousarray(hard_clusters, dtype=np.int8)).to(self.device)
            d_ham, d_wu = torch.from_numpy(ham).to(self.device), torch.from_numpy(wu).to(self.device)
            out = torch.empty((T, K), device=self.device, dtype=torch.float32)
            _call("dzn_speaker_scores", soft_device, hard, self.C, self.L, self.S, self.starts, d_ham, d_wu, T, K, out)
            return SlidingWindowFeature(out.cpu().numpy(), self.grid)


# ----------------------------------------------------------------------------- detection (VAD / OSD) scores
DETECT_SPEECH, DETECT_OVERLAP = 1, 2       # dzn_detect task bits (include/dzn.h)


def detection_hook(task: int, scores: np.ndarray) -> np.ndarray:
    """the pre-aggregation hooks of the two detection pipelines on [C, L, S] scores: max over speakers
    (PA/pipelines/voice_activity_detection.py:125) / second largest (PA/pipelines/overlapped_speech_detection.py:132)"""
    if task == DETECT_SPEECH:
        return np.max(scores, axis=-1, keepdims=True)
    return np.partition(scores, -2, axis=-1)[:, :, -2, np.newaxis]


def detection_weights(L: int, duration: float, warm_up=(0.0, 0.0), epsilon: float = 1e-12) -> np.ndarray:
    """float64 [L]: the Hamming window times the warm-up window of Inference.aggregate (PA/core/inference.py:590-611, warm_up in
    seconds), the factors a decision of 1 is multiplied with (a 0 contributes 0)"""
    ham = np.hamming(L).reshape(-1, 1)
    wu = np.ones((L, 1))
    left = round(warm_up[0] / duration * L)
    wu[:left] = epsilon
    right = round(warm_up[1] / duration * L)
    wu[L - right:] = epsilon
    return np.ascontiguousarray((ham * wu).reshape(-1), dtype=np.float64)


def crop_end(n: int, frames: SlidingWindow, end: float) -> int:
    """number of leading frames kept by SlidingWindowFeature.crop(Segment(0, end), mode="loose") on a grid starting at 0
    (PA/core/inference.py:400-403; pyannote.core SlidingWindow.crop: j = floor((end - start) / step), frames 0 .. j kept,
    clipped to the data)"""
    j = int(np.floor((end - frames.start) / frames.step))
    return max(0, min(j + 1, n))


def detection_scores_host(seg: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, task: int,
                          num_samples: Optional[int] = None, sample_rate: int = 16000) -> SlidingWindowFeature:
    """the numpy composition of the detection scores (Inference.__call__ with a pre-aggregation hook,
    PA/core/inference.py:389-403): hook -> aggregate(hamming=True, missing=0.0) -> crop when the last window was zero-padded
    (num_samples given and not on the step grid).  The device path (dzn_detect) is checked against it."""
    agg = aggregate(detection_hook(task, seg.astype(np.float32)), chunks, frames, hamming=True, missing=0.0)
    if num_samples is not None:
        window, step = int(np.floor(chunks.duration * sample_rate)), int(round(chunks.step * sample_rate))
        if num_samples < window or (num_samples - window) % step > 0:
            agg.data = agg.data[:crop_end(len(agg.data), agg.sliding_window, num_samples / sample_rate)]
    return agg


def detect_device(seg, chunks: SlidingWindow, frames: SlidingWindow, tasks: int, num_frames: Optional[int] = None,
                  onset: float = 0.5, offset: Optional[float] = None, want_scores: bool = False, warm_up=(0.0, 0.0),
                  frame_range: Optional[Tuple[int, int]] = None, entry=None):
    """dzn_detect on the current stream: seg u8 [C, L, S] (device tensor or host array) -> (activity u8 [T, K] host,
    scores f32 [T, K] host or None, frame grid).  T = num_frames (the cropped length) or the full aggregate length; the
    window start frames and the weight table are computed on the host with the reference's float64 arithmetic.
    frame_range = (t0, t1): dzn_detect_range instead — only frames t0 .. t1 - 1 (rows t - t0 of the two arrays), the
    hysteresis continuing from `entry`, u8 [K]: the activity of frame t0 - 1 (needed when t0 > 0)."""
    import torch
    offset = onset if offset is None else offset
    seg_t = seg if isinstance(seg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(seg, dtype=np.uint8)).cuda()
    assert seg_t.is_cuda and seg_t.dtype == torch.uint8 and seg_t.is_contiguous()
    dev = seg_t.device
    Cn, L, S = seg_t.shape
    grid, starts, T = _frame_grid(Cn, L, chunks, frames)
    T = T if num_frames is None else int(num_frames)
    K = bin(tasks & 3).count("1")
    with torch.cuda.device(dev):
        d_start = torch.from_numpy(starts).to(dev, non_blocking=False)
        d_w = torch.from_numpy(detection_weights(L, chunks.duration, warm_up)).to(dev)
        if frame_range is None:
            scores = torch.empty((T, K), device=dev, dtype=torch.float32)
            active = torch.empty((T, K), device=dev, dtype=torch.uint8)
            _call("dzn_detect", seg_t, Cn, L, S, d_start, d_w, T, tasks, float(np.float32(onset)), float(np.float32(offset)),
                  scores, active)
        else:
            t0, t1 = int(frame_range[0]), int(frame_range[1])
            d_entry = None
            if entry is not None:
                d_entry = torch.from_numpy(np.ascontiguousarray(entry, dtype=np.uint8).reshape(K)).to(dev)
            scores, active = detect_range_launch(seg_t, Cn, d_start, d_w, t0, t1, tasks, onset, offset, d_entry)
        act = active.cpu().numpy()
        sc = scores.cpu().numpy() if want_scores else None
    return act, sc, grid


def detect_range_launch(seg_t, num_windows: int, d_start, d_weight, t0: int, t1: int, tasks: int, onset: float, offset: float,
                        d_entry):
    """one dzn_detect_range call on the current stream over device operands: seg_t u8 [>= num_windows, L, S], d_start int32
    [>= num_windows], d_weight f64 [L], d_entry u8 [K] or None -> (scores f32 [t1 - t0, K], activity u8 [t1 - t0, K]), both
    device tensors.  Enqueue only."""
    import torch
    dev = seg_t.device
    _, L, S = seg_t.shape
    K = bin(tasks & 3).count("1")
    n = max(int(t1) - int(t0), 0)
    scores = torch.empty((n, K), device=dev, dtype=torch.float32)
    active = torch.empty((n, K), device=dev, dtype=torch.uint8)
    if n == 0:
        return scores, active                   # nothing to compute (an empty tensor has no address to hand over)
    _call("dzn_detect_range", seg_t, int(num_windows), L, S, d_start, d_weight, int(t0), int(t1), tasks,
          float(np.float32(onset)), float(np.float32(offset)), d_entry, scores, active)
    return scores, active


def diarize_range_launch(seg_t, hard_t, num_windows: int, d_start, t0: int, t1: int, K: int, max_count: int,
                         want_activations: bool = False):
    """one dzn_diarize_range call on the current stream over device operands: seg_t u8 [>= num_windows, L, S], hard_t int8
    [>= num_windows, S], d_start int32 [>= num_windows] -> (count u8 [t1 - t0], active u8 [t1 - t0, K], activations int32
    [t1 - t0, K] or None), device tensors.  Enqueue only."""
    import torch
    dev = seg_t.device
    _, L, S = seg_t.shape
    assert seg_t.is_cuda and seg_t.dtype == torch.uint8 and seg_t.is_contiguous()
    assert hard_t.is_cuda and hard_t.dtype == torch.int8 and hard_t.is_contiguous() and hard_t.shape[1] == S
    assert d_start.dtype == torch.int32 and min(len(seg_t), len(hard_t), len(d_start)) >= int(num_windows)
    n = max(int(t1) - int(t0), 0)
    count = torch.empty((n,), device=dev, dtype=torch.uint8)
    active = torch.empty((n, int(K)), device=dev, dtype=torch.uint8)
    act = torch.empty((n, int(K)), device=dev, dtype=torch.int32) if want_activations else None
    if n == 0:
        return count, active, act               # nothing to compute (an empty tensor has no address to hand over)
    _call("dzn_diarize_range", seg_t, hard_t, int(num_windows), L, S, d_start, int(t0), int(t1), int(K), int(max_count),
          count, active, act)
    return count, active, act


def diarize_range_scores_launch(seg_t, hard_t, soft_t, num_windows: int, d_start, d_ham, d_wu, t0: int, t1: int, K: int,
                                max_count: int, want_activations: bool = False):
    """one dzn_diarize_range_scores call on the current stream over device operands: those of diarize_range_launch, soft_t
    f32 [>= num_windows, L, S] and the two float64 [L] tables of aggregation_windows -> (count u8 [t1 - t0], active u8
    [t1 - t0, K], activations int32 [t1 - t0, K] or None, scores f32 [t1 - t0, K]), device tensors.  Enqueue only."""
    import torch
    dev = seg_t.device
    _, L, S = seg_t.shape
    assert seg_t.is_cuda and seg_t.dtype == torch.uint8 and seg_t.is_contiguous()
    assert hard_t.is_cuda and hard_t.dtype == torch.int8 and hard_t.is_contiguous() and hard_t.shape[1] == S
    assert soft_t.is_cuda and soft_t.dtype == torch.float32 and soft_t.is_contiguous() and tuple(soft_t.shape[1:]) == (L, S)
    assert d_start.dtype == torch.int32 and min(len(seg_t), len(hard_t), len(soft_t), len(d_start)) >= int(num_windows)
    assert d_ham.dtype == torch.float64 and d_wu.dtype == torch.float64 and len(d_ham) == L and len(d_wu) == L
    n = max(int(t1) - int(t0), 0)
    count = torch.empty((n,), device=dev, dtype=torch.uint8)
    active = torch.empty((n, int(K)), device=dev, dtype=torch.uint8)
    act = torch.empty((n, int(K)), device=dev, dtype=torch.int32) if want_activations else None
    scores = torch.empty((n, int(K)), device=dev, dtype=torch.float32)
    if n == 0:
        return count, active, act, scores       # nothing to compute (an empty tensor has no address to hand over)
    _call("dzn_diarize_range_scores", seg_t, hard_t, soft_t, int(num_windows), L, S, d_start, d_ham, d_wu, int(t0), int(t1),
          int(K), int(max_count), count, active, act, scores)
    return count, active, act, scores


def diarize_range_host(seg: np.ndarray, hard: np.ndarray, starts: np.ndarray, t0: int, t1: int, K: int, max_count: int):
    """numpy restatement of dzn_diarize_range (needs no device; the kernel is checked against it): seg u8 [C, L, S], hard
    [C, S], starts int [C] -> (count u8 [t1 - t0], active u8 [t1 - t0, K], activations int32 [t1 - t0, K])"""
    C, L, S = seg.shape
    T = max(int(t1), int(starts[-1]) + L if C else 0)
    tot, cover = np.zeros(T, np.int64), np.zeros(T, np.int64)
    act = np.zeros((T, K), np.int32)
    for c in range(C):
        s0 = int(starts[c])
        tot[s0:s0 + L] += seg[c].sum(axis=1, dtype=np.int64)
        cover[s0:s0 + L] += 1
        for k in range(K):
            sel = hard[c] == k
            if sel.any():
                act[s0:s0 + L, k] += seg[c][:, sel].max(axis=1)
    avg = np.where(cover > 0, tot.astype(np.float32) / np.maximum(cover, 1).astype(np.float32), np.float32(0))
    count = np.minimum(np.rint(avg).astype(np.uint8).astype(np.int64), int(max_count))
    order = np.argsort(-act, axis=1, kind="stable")
    active = np.zeros((T, K), np.uint8)
    np.put_along_axis(active, order, (np.arange(K)[None, :] < np.minimum(count, K)[:, None]).astype(np.uint8), axis=1)
    return count[t0:t1].astype(np.uint8), active[t0:t1], act[t0:t1]


def _select_top_count(act: SlidingWindowFeature, count: SlidingWindowFeature):
    """tail of to_diarization (PA/pipelines/utils/diarization.py:222-239) on aggregated activations"""
    K = act.data.shape[1]
    max_per_frame = int(np.max(count.data)) if count.data.size else 0
    if K < max_per_frame:
        act.data = np.pad(act.data, ((0, 0), (0, max_per_frame - K)))
    n = min(len(act.data), len(count.data))      # identical grids: extent & extent keeps all frames
    a = act.data[:n]
    c = count.data[:n].reshape(-1).astype(np.int64)
    binary = _top_count_mask(a, c)
    sw = SlidingWindow(start=act.sliding_window.start, duration=act.sliding_window.duration,
                       step=act.sliding_window.step)
    return SlidingWindowFeature(binary, sw), SlidingWindowFeature(a, sw)


def _top_count_mask(a: np.ndarray, c: np.ndarray) -> np.ndarray:
    """binary[i, k] = 1 for the c[i] largest activations of frame i — the reference sorts every frame
    (`np.argsort(-activations, axis=-1)` + a loop, PA/pipelines/utils/diarization.py:228-236), which is 0.07 s (AVX-512 host)
    to 0.6 s (without) of the 4 h host stage.  The selected SET does not depend on the sort when the c-th and (c+1)-th
    largest values of a frame differ: it is `a >= (c-th largest)`.  Only frames with a tie AT that boundary take the
    reference's own call, so its (numpy-build-dependent) tie order is reproduced, not re-invented."""
    n, K = a.shape
    binary = np.zeros_like(a)
    maxc = int(c.max()) if n else 0
    if maxc <= 0 or K == 0:
        return binary
    if maxc >= K:                                   # (count is capped at the number of columns by the padding above)
        maxc = K
    top = np.partition(a, K - maxc, axis=1)[:, K - maxc:]        # the maxc largest of every frame, unordered
    top = -np.sort(-top, axis=1)                                  # descending: top[:, j] = (j + 1)-th largest
    cc = np.minimum(c, K)
    kth = np.where(cc > 0, top[np.arange(n), np.maximum(cc, 1) - 1], np.inf)
    ge = a >= kth[:, None]
    clean = ge.sum(axis=1) == cc                    # no tie at the boundary: the set is unique
    binary[ge & clean[:, None]] = 1
    tied = np.nonzero(~clean & (cc > 0))[0]
    if len(tied):
        at = a[tied]
        order = np.argsort(-at, axis=-1)            # same call as the reference (ties: numpy's order)
        sel = (np.arange(K)[None, :] < cc[tied][:, None]).astype(a.dtype)
        bt = np.zeros_like(at)
        np.put_along_axis(bt, order, sel, axis=-1)
        binary[tied] = bt
    return binary


def binarize(diar: SlidingWindowFeature, onset: float = 0.5, offset: Optional[float] = None,
             uri: Optional[str] = None) -> Annotation:
    """Binarize(onset=0.5, offset=0.5, min_duration_on=0, min_duration_off=0): regions run from the
    MIDDLE of the first active frame to the middle of the first inactive frame (or of the last frame)."""
    offset = onset if offset is None else offset
    data = diar.data
    n, K = data.shape
    act = np.zeros((n, K), dtype=bool)
    if n >= 2:
        for k in range(K):
            y = data[:, k]
            # hysteresis state machine; with onset == offset on {0,1} data it is a plain threshold
            if onset == offset:
                act[:, k] = y > onset
                # frames exactly equal to the threshold keep the previous state
                if (y == onset).any():
                    act[:, k] = _hysteresis(y, onset, offset)
            else:
                act[:, k] = _hysteresis(y, onset, offset)
    return activity_regions(act, diar.sliding_window, uri=uri)


def activity_regions(active: np.ndarray, fr: SlidingWindow, uri: Optional[str] = None, labels=None) -> Annotation:
    """the region half of Binarize (PA/utils/signal.py:270-300) on precomputed per-frame activity [n, K]: a region runs
    from the middle of the frame that switched on to the middle of the frame that switched off (or of the last frame).
    Column k becomes track k with label `labels[k]` (default k)."""
    n, K = active.shape
    # frames[i].middle with pyannote.core's exact float64 op order (the .3f RTTM rounding of the
    # x.xxx5 timestamps depends on it): s = start + i*step ; e = s + duration ; middle = .5*(s + e)
    s_ = fr.start + np.arange(n) * fr.step
    ts = 0.5 * (s_ + (s_ + fr.duration))
    ann = Annotation(uri=uri)
    if n < 2:
        return ann
    fast = not HAVE_PYANNOTE_CORE and type(ann).__setitem__ is Annotation.__setitem__ and hasattr(ann, "_tracks")
    for k in range(K):
        act = active[:, k]
        label = k if labels is None else labels[k]
        d = np.diff(act.astype(np.int8))
        starts = np.nonzero(d == 1)[0] + 1
        ends = np.nonzero(d == -1)[0] + 1
        if act[0]:
            starts = np.concatenate([[0], starts])
        if act[-1]:
            ends = np.concatenate([ends, [n - 1]])
        # 30 k turns at 4 h: the python objects are the cost (r6 profile: 75 ms); timestamps leave numpy in one tolist() each and
        # the stand-in Annotation (core.py) is filled through its dictionary - same entries as `ann[Segment(s, e), k] = k`
        t0, t1 = ts[starts].tolist(), ts[ends].tolist()
        if fast:
            tracks = ann._tracks
            for a, b in zip(t0, t1):
                if b > a:                     # pyannote ignores empty segments
                    tracks.setdefault(Segment(a, b), {})[k] = label
        else:
            for a, b in zip(t0, t1):
                ann[Segment(a, b), k] = label
    return ann


def _hysteresis(y: np.ndarray, onset: float, offset: float) -> np.ndarray:
    act = np.zeros(len(y), dtype=bool)
    state = y[0] > onset
    act[0] = state
    for i in range(1, len(y)):
        if state:
            if y[i] < offset:
                state = False
        elif y[i] > onset:
            state = True
        act[i] = state
    return act


# ----------------------------------------------------------------------------- resegmentation: matching to a given diarization
MATCH_MAX_N = 32            # dzn_match_counts' widest padded side (include/dzn.h)


def trim_frames(L: int, warm_up: float) -> Tuple[int, int]:
    """(l0, L'): frames [l0, l0 + L') of every window survive Inference.trim(warm_up=(w, w)) (PA/core/inference.py:696-705)"""
    l0 = round(L * warm_up)
    return int(l0), int(L - 2 * l0)


def trimmed_chunks(chunks: SlidingWindow, warm_up: float) -> SlidingWindow:
    """the chunks of the trimmed windows (PA/core/inference.py:707-711): window c becomes [c step + w D, c step + (1 - w) D)"""
    return SlidingWindow(start=chunks.start + warm_up * chunks.duration, step=chunks.step,
                         duration=(1 - warm_up - warm_up) * chunks.duration)


def reference_extent(num_samples: int, sample_rate: int, chunks: SlidingWindow, frames: SlidingWindow) -> Tuple[int, int]:
    """(f0, Tr) of the discretised hypothesis: support Segment(0, duration + step) on the model's frames
    (PA/pipelines/resegmentation.py:203-208), f0 = closest_frame(0), Tr = closest_frame(duration + step) - f0"""
    f0 = int(frames.closest_frame(0.0))
    return f0, max(int(frames.closest_frame(num_samples / sample_rate + chunks.step)) - f0, 0)


def reference_rows(C: int, chunks: SlidingWindow, frames: SlidingWindow) -> np.ndarray:
    """int32 [C]: the first reference row of every (trimmed) window — the first frame of SlidingWindowFeature.crop(chunk),
    mode "loose" (PA/pipelines/resegmentation.py:234): max(0, ceil((chunk.start - frames.duration - frames.start) / step))"""
    starts = chunks.start + np.arange(C, dtype=np.float64) * chunks.step
    r = np.ceil((starts - frames.duration - frames.start) / frames.step)
    return np.maximum(r, 0).astype(np.int32)


def annotation_turns(annotation) -> list:
    """[(start, end, label)] of an Annotation (or of a list of such triples, der.parse_rttm's form), in its own order"""
    if hasattr(annotation, "itertracks"):
        return [(float(s.start), float(s.end), label) for s, _, label in annotation.itertracks(yield_label=True)]
    return [(float(a), float(b), label) for a, b, label in annotation]


def discretize_turns(annotation, frames: SlidingWindow, Tr: int):
    """-> (ref u8 [Tr, K], labels): the hypothesis on the frame grid, as Annotation.discretize(support=Segment(0, end),
    resolution=frames) of pyannote.core 5.0.0 does it (restated: that package is not a dependency, the boundary is unpinned).
    labels = the input's labels sorted by str(), column k = labels[k].  A turn [a, b) sets rows max(0, closest_frame(a) - f0)
    .. min(closest_frame(b) - f0, Tr - 1), f0 = closest_frame(0) (SlidingWindow.crop(mode="center")); turns that end at or
    before 0 are outside the support."""
    turns = annotation_turns(annotation)
    labels = sorted({label for _, _, label in turns}, key=str)
    col = {label: k for k, label in enumerate(labels)}
    Tr = max(int(Tr), 0)
    ref = np.zeros((Tr, len(labels)), dtype=np.uint8)
    f0 = int(frames.closest_frame(0.0))
    for a, b, label in turns:
        if b <= 0.0 or b <= a:
            continue
        lo = max(0, int(frames.closest_frame(a)) - f0)
        hi = min(int(frames.closest_frame(b)) - f0, Tr - 1)
        if hi >= lo:
            ref[lo:hi + 1, col[label]] = 1
    return ref, labels


def match_counts_host(seg: np.ndarray, ref: np.ndarray, rows: np.ndarray, l0: int, Lt: int, K: int) -> np.ndarray:
    """numpy twin of dzn_match_counts (needs no device; the kernel is checked against it): seg u8 [C, L, S], ref u8 [Tr, K],
    rows int [C] -> int32 [C, n, n], n = max(K, S): count[c, i, j] = #{l < Lt : refpad[rows[c] + l, i] != segpad[c, l0 + l, j]},
    both sides widened to n columns with zeros, reference rows at or beyond Tr zero"""
    seg = np.asarray(seg)
    C, L, S = seg.shape
    K, l0, Lt = int(K), int(l0), int(Lt)
    n = max(K, S)
    if Lt < 1 or l0 < 0 or l0 + Lt > L:
        raise ValueError(f"frames [{l0}, {l0 + Lt}) are not inside a window of {L}")
    ref = np.asarray(ref) != 0
    assert ref.ndim == 2 and ref.shape[1] == K
    Tr = len(ref)
    out = np.zeros((C, n, n), dtype=np.int32)
    sp = np.zeros((Lt, n), dtype=bool)
    for c in range(C):
        rp = np.zeros((Lt, n), dtype=bool)
        r = int(rows[c])
        a, b = min(max(r, 0), Tr), min(max(r + Lt, 0), Tr)
        if b > a:
            rp[a - r:b - r, :K] = ref[a:b]
        sp[:, :S] = seg[c, l0:l0 + Lt] != 0
        out[c] = np.count_nonzero(rp[:, :, None] != sp[:, None, :], axis=0)
    return out


def match_counts_device(seg_t, ref, rows: np.ndarray, l0: int, Lt: int, K: int) -> np.ndarray:
    """dzn_match_counts on the current stream: seg_t u8 [C, L, S] on the device, ref u8 [Tr, K] (host array or device tensor),
    rows int [C] -> int32 [C, n, n] on the host.  Only the counts come back."""
    import torch
    assert seg_t.is_cuda and seg_t.dtype == torch.uint8 and seg_t.is_contiguous()
    dev = seg_t.device
    C, L, S = (int(d) for d in seg_t.shape)
    K = int(K)
    n = max(K, S)
    with torch.cuda.device(dev):
        if not isinstance(ref, torch.Tensor):
            ref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.uint8)).to(dev)
        assert ref.dtype == torch.uint8 and ref.is_contiguous() and ref.dim() == 2 and ref.shape[1] == K
        Tr = int(ref.shape[0])
        d_row = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        assert len(d_row) == C
        out = torch.empty((C, n, n), device=dev, dtype=torch.int32)
        _call("dzn_match_counts", seg_t, ref if ref.numel() else None, C, L, S, Tr, K, d_row, int(l0), int(Lt), out)
        return out.cpu().numpy()


def assign_windows(counts: np.ndarray, Lt: int, S: int) -> np.ndarray:
    """int32 counts [C, n, n] -> hard int8 [C, S]: hard[c, j] = i, the speaker of the hypothesis that local speaker j of
    window c is matched to.  cost = float32(count) / float32(Lt) (mae_cost_func's torch.mean, PA/utils/permutation.py:83-95),
    then scipy.optimize.linear_sum_assignment per window (permutation.py:152-156)."""
    from scipy.optimize import linear_sum_assignment
    cost = (counts.astype(np.float32) / np.float32(Lt)).astype(np.float64)
    hard = np.zeros((len(counts), int(S)), dtype=np.int8)
    for c in range(len(counts)):
        i, j = linear_sum_assignment(cost[c])
        keep = j < S
        hard[c, j[keep]] = i[keep]
    return hard


def permutated_decisions(trimmed: np.ndarray, hard: np.ndarray, n: int) -> np.ndarray:
    """the permutated segmentations of PA/pipelines/resegmentation.py:231-243 as float32 [C, L', n]: column hard[c, j] of
    window c is local speaker j, the other columns (matched to padded local speakers) are zero"""
    C, Lt, S = trimmed.shape
    out = np.zeros((C, Lt, int(n)), dtype=np.float32)
    cc = np.arange(C)
    for j in range(S):
        out[cc, :, hard[:, j].astype(np.int64)] = trimmed[:, :, j]
    return out


def resegment_host(seg: np.ndarray, ref: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, warm_up: float = 0.0):
    """the host composition of PA/pipelines/resegmentation.py:184-246 on hard decisions seg u8 [C, L, S] and a discretised
    hypothesis ref u8 [Tr, K] -> (speaker count [T, 1], counts int32 [C, n, n], hard int8 [C, S], discrete diarization [T, n']).
    Needs no device; the device path of resegmentation.Resegmentation is checked against it."""
    seg = np.ascontiguousarray(seg, dtype=np.uint8)
    C, L, S = seg.shape
    ref = np.asarray(ref, dtype=np.uint8)
    K = int(ref.shape[1])
    n = max(K, S)
    l0, Lt = trim_frames(L, warm_up)
    tc = trimmed_chunks(chunks, warm_up) if warm_up else chunks
    trimmed = seg[:, l0:l0 + Lt]
    count = speaker_count(trimmed.astype(np.float32), tc, frames)
    counts = match_counts_host(seg, ref, reference_rows(C, tc, frames), l0, Lt, K)
    hard = assign_windows(counts, Lt, S)
    discrete, _ = to_diarization(permutated_decisions(trimmed, hard, n), tc, count)
    return count, counts, hard, discrete


def resegment_device(seg_t, ref: np.ndarray, chunks: SlidingWindow, frames: SlidingWindow, warm_up: float = 0.0, step=None):
    """resegment_host over decisions u8 [C, L, S] that are on the device, same return value, same bits.  The matching counts
    are dzn_match_counts'; with warm_up == 0 the speaker count and the aggregation of the matched decisions are DevicePost's
    (dzn_speaker_count, dzn_cluster_activations), with warm_up > 0 they are the numpy functions on the trimmed download.  More
    than MATCH_MAX_N speakers on the wider side: resegment_host on the download (the K > 32 rule of DevicePost.reconstruct).
    step(name, artifact): called with "speaker_counting" and "permutated" as they become available."""
    step = step or (lambda *a: None)
    C, L, S = (int(d) for d in seg_t.shape)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    K = int(ref.shape[1])
    n = max(K, S)
    if n > MATCH_MAX_N:
        count, counts, hard, discrete = resegment_host(seg_t.cpu().numpy(), ref, chunks, frames, warm_up)
        step("speaker_counting", count)
        step("permutated", hard)
        return count, counts, hard, discrete
    l0, Lt = trim_frames(L, warm_up)
    tc = trimmed_chunks(chunks, warm_up) if warm_up else chunks
    rows = reference_rows(C, tc, frames)
    if warm_up:
        trimmed = seg_t.cpu().numpy()[:, l0:l0 + Lt]
        count = speaker_count(trimmed.astype(np.float32), tc, frames)
        step("speaker_counting", count)
        counts = match_counts_device(seg_t, ref, rows, l0, Lt, K)
        hard = assign_windows(counts, Lt, S)
        step("permutated", hard)
        discrete, _ = to_diarization(permutated_decisions(trimmed, hard, n), tc, count)
        return count, counts, hard, discrete
    post = DevicePost.from_device(seg_t, chunks, frames)
    count = post.speaker_count()
    step("speaker_counting", count)
    counts = match_counts_device(seg_t, ref, rows, 0, L, K)
    hard = assign_windows(counts, L, S)
    step("permutated", hard)
    discrete, _ = post.reconstruct(hard, count, num_clusters=n)
    return count, counts, hard, discrete
