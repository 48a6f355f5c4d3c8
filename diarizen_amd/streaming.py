"""Streaming / online use of the hot path (row f3 of SURVEY §8f: "window scheduler": PA/core/inference.py:316-343 batches
windows of a file that is already complete; here windows are scheduled AS THE AUDIO ARRIVES).

    for t, annotation in pipeline.stream(chunks, sess_name="meeting"):      # chunks: iterable of float32 arrays
        ...                                                                 # provisional turns up to t seconds
    # the last item is the final annotation — byte-identical RTTM to pipeline(<the whole file>)

Design (MI355X-first, same kernels as the offline path):
  * ingest: every chunk lands in a slot of a PINNED host ring and is copied to the device on a dedicated copy stream
    (`non_blocking` H2D, one event per slot); the compute stream only waits for the event of the newest slot a window
    needs, so upload and compute overlap and the caller's buffer is free as soon as feed() returns;
  * a session opened with `feed_format=audio.FeedFormat(8000, "ulaw", channels=2)` is fed the source's own bytes instead —
    G.711 / PCM frames at 8 .. 48 kHz in packets of any length: the ring then holds stored frames, each slot has a device
    twin, and dzn_resample (dzn_decode at the model's rate) writes the samples that have become final (audio.feed_ready)
    straight into the device buffer, on the copy stream; the waveform is resample_device of the whole recording bit for bit;
  * a microphone ARRAY (`FeedFormat(16000, "s16", channels=8, channel=Beamform(causal=True))`, or a pipeline built with that
    channel) is beamformed inside the same ingest: per planned call dzn_beamform_feed enqueues the planar decode, GCC-PHAT of the
    newly complete blocks, the device delay tracker and delay-and-sum on the copy stream (csrc/beamform_live.hip); the waveform
    is the offline BeamformedSource of the whole recording bit for bit;
  * the device holds the recording so far in ONE pre-zeroed buffer (4 h of 16 kHz mono = 0.92 GB of the 288 GB); windows are
    rows of a strided view over it, exactly as offline (inference.WindowRunner), so a window is computed once, when its last
    sample has arrived, and never again.  Samples past the end read as zeros: the reference's zero-padded last window
    (PA/core/inference.py:293-299) needs no special case at finish();
  * per-window results are batch-invariant (tests/test_properties_gpu.py), hence the streamed decisions / embeddings —
    and the final RTTM — equal the offline ones bit for bit;
  * provisional output: every `refresh_s` seconds of new audio the host stage (counting, clustering, reconstruction,
    Binarize) runs over the windows finished so far.  Speaker labels of provisional annotations are NOT stable across
    refreshes (each is a fresh clustering), the final one is the offline result.  Labels that never change and a committed
    prefix are what live.LiveDiarization (pipeline.open_live) gives instead, on the same ingest.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, Iterator, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import audio as audio_io
from . import dist as dz_dist
from .core import Annotation
from .inference import window_plan
from .postprocess import _frame_grid, committed_frames, covered_frames, receptive_field


def complete_windows(num_samples: int, window: int, step: int) -> int:
    """windows whose last sample has arrived (the zero-padded tail window only exists once the stream has ended)"""
    return 0 if num_samples < window else (num_samples - window) // step + 1


def plan_feed(fmt, sample_rate: int, slot_frames: int, tile: Optional[int] = None):
    """the audio.FeedPlanner of a stored-format feed (at most `slot_frames` new source frames per planned call), or the
    refusal, by name and before any allocation, of a format the device ingest cannot serve (WaveIngest, hub.LiveHub);
    tile: the device resampler's tile (default: asked of the library)"""
    if not isinstance(fmt, audio_io.FeedFormat) or fmt.channel is None:
        raise ValueError(f"feed_format is an audio.FeedFormat with a channel choice, not {fmt!r}")
    if isinstance(fmt.channel, audio_io.Beamform):                       # an array feed: beamformed inside the ingest
        plan = audio_io.ArrayFeedPlanner(fmt, sample_rate, slot_frames)
    else:
        plan = audio_io.FeedPlanner(fmt, sample_rate, slot_frames)
    if not plan.same_rate and not audio_io.resample_tile_fits(plan.o, plan.n, plan.width, tile or audio_io.resample_tile()):
        raise ValueError(f"feed_format: {fmt.rate} Hz -> {sample_rate} Hz (o / n = {plan.o} / {plan.n}): the input of one "
                         "tile of the device resampler does not fit in LDS")
    return plan


class WaveIngest:
    """The ingest half of a streaming session (WindowStream): a PINNED host ring,
    a dedicated copy stream and ONE pre-zeroed device buffer that holds the recording so far; `views` are its windows as rows
    of a strided view.  append() stages a chunk slot by slot and queues the H2D copies; wait() makes the current stream wait
    for the newest one.

    With a `feed_format` (audio.FeedFormat, its channel settled) append() takes the source's own bytes — G.711 or PCM frames
    at 8 .. 48 kHz — instead of float32 samples.  audio.FeedPlanner says what each chunk makes final; per planned call the
    slot holds [history | new frames] as stored, is copied to its DEVICE TWIN on copy_stream, and on the same stream ONE
    dzn_resample call (dzn_decode for a feed at the model's rate) writes the output samples [ready before, ready after)
    straight into dev_wave.  The slot's event is recorded after the kernel, so reusing a slot waits for the kernel that read
    its twin.  `n` counts the model-rate samples that are final, `frames` the source frames received; flush() makes the tail
    once the stream has ended.  dev_wave[:n] is then resample_device of the whole recording, bit for bit.

    An ARRAY feed (`FeedFormat(..., channel=Beamform(causal=True))`, audio.ArrayFeedPlanner) uses the same ring, twins and slot
    events; per planned call ONE dzn_beamform_feed enqueues, on copy_stream, the planar decode of the uploaded frames, GCC-PHAT
    of the newly complete blocks, the delay tracker and the delay-and-sum of the samples that became final
    (audio.beam_ready) — straight into dev_wave, or, where the rates differ, behind the carried history of one of two small
    staging buffers that dzn_resample then reads.  The tracker state and the delay table live on the device; nothing is read
    back (`delays()` is the one call that synchronises).  dev_wave[:n] is then BeamformedSource.read_device of the whole
    recording with the same Beamform, bit for bit."""

    def __init__(self, device, sample_rate: int, window: int, step: int, max_seconds: float = 4 * 3600.0,
                 slot_seconds: float = 10.0, slots: int = 4, feed_format=None, slot_frames: Optional[int] = None):
        """feed_format: an audio.FeedFormat with a channel; slot_frames: new source frames per slot (default: slot_seconds of
        the feed)"""
        self.plan = None
        if feed_format is not None:
            self._open_format(feed_format, sample_rate, slot_seconds, slot_frames)      # refusals before any allocation
        self.device = device
        self.sr = sample_rate
        self.window = window
        self.capacity = int(max_seconds * self.sr) + window             # + one window of zeros behind the last sample
        self.dev_wave = torch.zeros(self.capacity, device=device, dtype=torch.float32)
        self.views = torch.as_strided(self.dev_wave, ((self.capacity - window) // step + 1, window), (step, 1))
        self.slot_samples = int(slot_seconds * self.sr)
        self.array = isinstance(self.plan, audio_io.ArrayFeedPlanner)
        if self.array:
            self._open_array(max_seconds)
        if self.plan is None:
            self.ring = [torch.empty(self.slot_samples, dtype=torch.float32).pin_memory() for _ in range(slots)]
        else:
            nbytes = self.plan.max_upload_frames * self.plan.fmt.frame_bytes
            self.ring = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self.ring_np = [r.numpy() for r in self.ring]               # views of the pinned slots
            self.twins = [torch.empty(nbytes, device=device, dtype=torch.uint8) for _ in range(slots)]
            if not self.plan.same_rate:
                self.bank = audio_io._device_bank(self.plan.fmt.rate, self.sr, device)[0]
        self.slot_free = [None] * slots                                 # event: the slot's H2D copy has completed
        self.next_slot = 0
        self.copy_stream = torch.cuda.Stream(device=device)
        # the zero fill of dev_wave above is queued on the CURRENT stream; the chunk copies run on copy_stream — without this
        # edge the first copies could land before the memset and be zeroed by it.  record_stream: the caching allocator
        # must not recycle dev_wave while copies on the other stream are pending.
        self.copy_stream.wait_stream(torch.cuda.current_stream(device))
        self.dev_wave.record_stream(self.copy_stream)
        if self.plan is not None:
            for t in self.twins:
                t.record_stream(self.copy_stream)
        if self.array:
            for t in [self._planar, self._lag, self._peak, self._state, self._delay, *self._stage]:
                t.record_stream(self.copy_stream)
        self.n = 0                                                      # samples received (a stored feed: samples that are final)
        self.frames = 0                                                 # source frames received (== n without a feed_format)
        self.uploads = 0
        self.last_copy = None

    def _open_format(self, fmt, sample_rate: int, slot_seconds: float, slot_frames: Optional[int]) -> None:
        if not isinstance(fmt, audio_io.FeedFormat):
            raise ValueError(f"feed_format is an audio.FeedFormat with a channel choice, not {fmt!r}")
        self.plan = plan_feed(fmt, sample_rate, int(slot_seconds * fmt.rate) if slot_frames is None else slot_frames)

    def _open_array(self, max_seconds: float) -> None:
        """the per-session device buffers of an array feed: planar scratch, lag / peak temporaries, tracker state (zeroed), delay
        table, and where the rates differ two staging buffers [history | new] of beamformed samples"""
        plan, device = self.plan, self.device
        C = plan.fmt.channels
        self._table_blocks = -(-(int(max_seconds * plan.fmt.rate) + 1) // plan.hop) + 2
        self._planar = torch.empty((C, plan.max_upload_frames), device=device, dtype=torch.float32)
        self._lag = torch.empty((C, plan.max_blocks), device=device, dtype=torch.int32)
        self._peak = torch.empty((C, plan.max_blocks), device=device, dtype=torch.float32)
        self._state = torch.zeros((C, 5), device=device, dtype=torch.int32)      # DZN_BEAMFORM_STATE_INTS
        self._delay = torch.zeros((C, self._table_blocks), device=device, dtype=torch.int32)
        self._twiddle = audio_io._device_twiddle(plan.hop, device)
        self._stage = [] if plan.same_rate else [torch.empty(plan.K + plan.max_new, device=device, dtype=torch.float32)
                                                 for _ in range(2)]
        self._stage_at, self._stage_first = 0, 0        # the buffer that holds beamformed samples _stage_first .. plan.ready
        import ctypes
        self._seen = ctypes.c_int64(0)                  # blocks tracked: the host's count that dzn_beamform_feed checks b0 by

    def delays(self) -> np.ndarray:
        """int32 [C, blocks]: the delay table of an array feed as far as it is filled (after flush(): of the whole recording).
        The one call of the ingest that waits for the device; append() and flush() never do."""
        if not self.array:
            raise ValueError("delays(): not an array feed")
        self.copy_stream.synchronize()
        return self._delay[:, :self.plan.blocks].cpu().numpy()

    def append(self, samples) -> int:
        """stage float32 samples and queue their copies behind the recording so far; -> number of samples taken.  With a
        feed_format: bytes (or an array of the stored dtype) of any length, also ending inside a frame; -> the number of
        samples that became final"""
        if self.plan is not None:
            data = audio_io._feed_bytes(samples, self.plan.fmt)
            if self.plan.length_after(len(data)) + self.window > self.capacity:
                raise MemoryError(f"stream longer than max_seconds = {(self.capacity - self.window) / self.sr:.0f} s")
            return self._run(self.plan.append(data))
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).reshape(-1))
        if self.n + len(x) + self.window > self.capacity:
            raise MemoryError(f"stream longer than max_seconds = {(self.capacity - self.window) / self.sr:.0f} s")
        off = 0
        while off < len(x):
            k = min(self.slot_samples, len(x) - off)
            i = self.next_slot
            if self.slot_free[i] is not None:
                self.slot_free[i].synchronize()                         # ring full: wait for the oldest copy only
            self.ring[i][:k].copy_(torch.from_numpy(x[off:off + k]))
            with torch.cuda.stream(self.copy_stream):
                self.dev_wave[self.n + off:self.n + off + k].copy_(self.ring[i][:k], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.slot_free[i] = ev
            self.last_copy = ev
            self.next_slot = (i + 1) % len(self.ring)
            self.uploads += 1
            off += k
        self.n += len(x)
        self.frames = self.n
        return len(x)

    def flush(self) -> int:
        """end of stream.  A stored feed: the samples [n, resampled_length(frames)) that waited for frames which will not come (a
        trailing partial frame is dropped); -> the number of samples added (0 without a feed_format)"""
        return 0 if self.plan is None else self._run(self.plan.finish())

    def _run(self, calls) -> int:
        """upload and launch the planned calls on copy_stream; -> output samples made"""
        import ctypes as C
        if self.array:
            return self._run_array(calls)
        lib, fmt, plan = _lib.load(), self.plan.fmt, self.plan
        device = torch.device(self.device)
        dev = device.index if device.index is not None else -1
        n0 = self.n
        for c in calls:
            nb = len(c.data)
            assert c.m0 == self.n and nb == c.frames * fmt.frame_bytes <= len(self.ring[0]) and c.m1 + self.window <= self.capacity
            i = self.next_slot
            if self.slot_free[i] is not None:
                self.slot_free[i].synchronize()                         # ring full: wait for the oldest copy and its kernel
            self.ring_np[i][:nb] = np.frombuffer(c.data, dtype=np.uint8)
            with torch.cuda.stream(self.copy_stream):
                self.twins[i][:nb].copy_(self.ring[i][:nb], non_blocking=True)
                st = C.c_void_p(self.copy_stream.cuda_stream)
                src, dst = C.c_void_p(self.twins[i].data_ptr()), C.c_void_p(self.dev_wave.data_ptr() + 4 * c.m0)
                if plan.same_rate:
                    _lib.check(lib.dzn_decode(dev, src, fmt.src_format, fmt.channels, fmt.channel_code(), c.frames, dst, st),
                               None, "dzn_decode")
                else:
                    _lib.check(lib.dzn_resample(dev, src, fmt.src_format, fmt.channels, fmt.channel_code(), c.first, c.frames,
                                                c.total, C.c_void_p(self.bank.data_ptr()), plan.o, plan.n, plan.width, c.m0,
                                                c.m1, dst, st), None, "dzn_resample")
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.slot_free[i] = ev
            self.last_copy = ev
            self.next_slot = (i + 1) % len(self.ring)
            self.uploads += 1
            self.n = c.m1
        self.frames = plan.frames
        return self.n - n0

    def _run_array(self, calls) -> int:
        """the planned calls of an array feed, enqueue-only on copy_stream: upload, dzn_beamform_feed, and where the rates
        differ the history carried into the other staging buffer and dzn_resample; -> output samples made"""
        import ctypes as C
        lib, fmt, plan = _lib.load(), self.plan.fmt, self.plan
        device = torch.device(self.device)
        dev = device.index if device.index is not None else -1
        vp = C.c_void_p
        made = self.n
        for c in calls:
            nb = len(c.data)
            assert (c.m0 == self.n and nb == c.frames * fmt.frame_bytes <= len(self.ring[0]) and c.m1 + self.window <= self.capacity
                    and c.b1 <= self._table_blocks and c.b1 - c.b0 <= plan.max_blocks and c.n1 - c.n0 <= plan.max_new)
            i = self.next_slot
            if self.slot_free[i] is not None:
                self.slot_free[i].synchronize()                         # ring full: wait for the oldest copy and its kernels
            self.ring_np[i][:nb] = np.frombuffer(c.data, dtype=np.uint8)
            with torch.cuda.stream(self.copy_stream):
                if nb:
                    self.twins[i][:nb].copy_(self.ring[i][:nb], non_blocking=True)
                st = vp(self.copy_stream.cuda_stream)
                dst, stage = self.dev_wave.data_ptr() + 4 * c.n0, None
                if not plan.same_rate and (c.n1 > c.n0 or c.m1 > c.m0):
                    old, stage = self._stage[self._stage_at], self._stage[self._stage_at ^ 1]
                    hist = c.n0 - c.s_first                             # < K beamformed samples a later range still reads
                    assert c.s_first >= self._stage_first and hist + c.n1 - c.n0 <= len(stage)
                    if hist:
                        stage[:hist].copy_(old[c.s_first - self._stage_first:c.n0 - self._stage_first], non_blocking=True)
                    dst = stage.data_ptr() + 4 * hist
                    self._stage_at, self._stage_first = self._stage_at ^ 1, c.s_first
                _lib.check(lib.dzn_beamform_feed(
                    dev, vp(self.twins[i].data_ptr()), fmt.src_format, fmt.channels, c.first, c.frames, c.total,
                    plan.beamform.reference, plan.hop, plan.max_lag, plan.min_peak, vp(self._twiddle.data_ptr()),
                    vp(self._planar.data_ptr()), self._planar.shape[1], vp(self._lag.data_ptr()), vp(self._peak.data_ptr()),
                    plan.max_blocks, c.b0, c.b1, vp(self._state.data_ptr()), C.byref(self._seen), vp(self._delay.data_ptr()),
                    self._table_blocks, c.n0, c.n1, vp(dst), st), None, "dzn_beamform_feed")
                if stage is not None and c.m1 > c.m0:
                    _lib.check(lib.dzn_resample(dev, vp(stage.data_ptr()), 0, 1, 0, c.s_first, c.n1 - c.s_first, c.n1,
                                                vp(self.bank.data_ptr()), plan.o, plan.n, plan.width, c.m0, c.m1,
                                                vp(self.dev_wave.data_ptr() + 4 * c.m0), st), None, "dzn_resample")
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.slot_free[i] = ev
            self.last_copy = ev
            self.next_slot = (i + 1) % len(self.ring)
            self.uploads += 1
            self.n = c.m1
        self.frames = plan.frames
        return self.n - made

    def wait(self) -> None:
        """the current (compute) stream runs behind the newest upload"""
        if self.last_copy is not None:
            torch.cuda.current_stream(self.device).wait_event(self.last_copy)


class WindowStream:
    """What every feed / finish session shares: the ingest, each complete window run ONCE through the runner (`_compute`; the
    subclass takes the results in `_windows`), the feed-after-finish guard, the reference's final-window rule and the RTTM file.

    A session opened by a hub (hub.LiveHub.open: `hub=`) is the same object with the hub's ingest — a row of the hub's pooled
    device buffer instead of a WaveIngest of its own — and its device work is driven by the hub's tick() instead of by feed():
    the three steps "stage" (`_append` / `_flush`: host only), "take results" (`_take`) and "advance" (`_step`) are what
    feed() / finish() of a solo session run back to back."""
    EMBEDDINGS = True                                                   # run_views(with_embeddings=...)
    SCORES = False                                                      # run_views(with_scores=True): the classifier's soft output too

    def __init__(self, pipeline, name: Optional[str] = None, max_seconds: float = 4 * 3600.0, slot_seconds: float = 10.0,
                 slots: int = 4, feed_format=None, hub=None):
        """pipeline: a DiariZenPipeline or a detection pipeline (its _runner, device and rttm_out_dir are used); name: the
        session name / uri of the annotations and of the RTTM file; feed_format: an audio.FeedFormat when the feeds are the
        source's own bytes (G.711 / PCM frames at its rate; a format without a channel takes the pipeline's) — refused here,
        not at the first feed, when it cannot be served; hub: the hub.LiveHub that owns the ingest and the device work (its
        max_seconds and staging ring hold, not these)"""
        self.pipe = pipeline
        self.hub = hub
        self.name = name
        self.runner = r = pipeline._runner
        self.sr = r.sample_rate
        self.device = pipeline.device
        with torch.cuda.device(self.device):
            if feed_format is not None:
                if not isinstance(feed_format, audio_io.FeedFormat):
                    raise ValueError(f"feed_format is an audio.FeedFormat, not {feed_format!r}")
                feed_format = feed_format.with_channel(getattr(pipeline, "channel", 0))
            self.feed_format = feed_format
            if hub is None:
                self.ingest = WaveIngest(self.device, self.sr, r.window, r.step, max_seconds, slot_seconds, slots, feed_format)
            else:
                self.ingest = hub._row_ingest(feed_format)              # refuses as WaveIngest does, then takes a pool row
        self.done = 0                                                   # windows computed
        self.finished = False
        self.stats = {"uploads": 0, "windows": 0, "launches": 0}

    @property
    def n(self) -> int:
        """samples received (with a feed_format: model-rate samples that are final)"""
        return self.ingest.n

    @property
    def seconds(self) -> float:
        """seconds of audio received (with a feed_format: of model-rate audio that is final; the feed is at most
        width + o - 1 source frames ahead, audio.feed_ready)"""
        return self.ingest.n / self.sr

    def _append(self, samples) -> int:
        """stage float32 samples (mono, the runner's rate), or bytes / stored-dtype arrays of the session's feed_format
        -> number of samples taken (that became final)"""
        if self.finished:
            raise RuntimeError("stream already finished")
        taken = self.ingest.append(samples)
        self.stats["uploads"] = self.ingest.uploads
        return taken

    def _compute(self, upto: int) -> None:
        """run windows done .. upto on the compute stream, behind the newest upload"""
        if upto <= self.done:
            return
        self.ingest.wait()
        kw = {"with_scores": True} if self.SCORES else {}
        self._take(self.runner.run_views(self.ingest.views, self.done, upto, with_embeddings=self.EMBEDDINGS, **kw), upto)

    def _take(self, res, upto: int) -> None:
        """take the results of windows done .. upto - 1 from the forward that ran them (here, or a hub's batch over many
        sessions)"""
        self._windows(res, self.done, upto)
        self.stats["launches"] += 1
        self.stats["windows"] += upto - self.done
        self.done = upto

    def _windows(self, res, lo: int, hi: int) -> None:
        """keep the results of windows lo .. hi - 1"""
        raise NotImplementedError

    def _flush(self) -> None:
        """end of stream: the samples of a stored feed that waited for frames which will not come"""
        self.ingest.flush()
        self.stats["uploads"] = self.ingest.uploads

    def _final_windows(self) -> Tuple[int, bool]:
        """(windows of the whole recording, the last of them is zero-padded): the reference's rule, PA/core/inference.py:293-299"""
        n_full, has_last = window_plan(self.n, self.runner.window, self.runner.step)
        return n_full + int(has_last), has_last

    def _write_rttm(self, ann: Annotation) -> None:
        """the final annotation as <rttm_out_dir>/<name>.rttm, when the pipeline has the one and the session the other"""
        if self.pipe.rttm_out_dir is not None and self.name is not None:
            with open(os.path.join(self.pipe.rttm_out_dir, self.name + ".rttm"), "w") as f:
                f.write(ann.to_rttm())


class StreamingSession(WindowStream):
    def __init__(self, pipeline, sess_name: Optional[str] = None, max_seconds: float = 4 * 3600.0, refresh_s: Optional[float] = 8.0,
                 slot_seconds: float = 10.0, slots: int = 4, feed_format=None, return_scores: bool = False):
        """return_scores=True: feed() / finish() give (Annotation, scores) — the per-speaker activity scores of
        `pipeline(file, return_scores=True)`; the windows' soft scores stay on the device across feeds (one device only)"""
        if not isinstance(return_scores, (bool, np.bool_)):
            raise ValueError(f"return_scores is True or False, not {return_scores!r}")
        if return_scores and dz_dist.world_size() > 1:
            raise RuntimeError(pipeline._ONE_DEVICE % ("stream(return_scores=True)", dz_dist.world_size()))
        self.SCORES = bool(return_scores)
        super().__init__(pipeline, sess_name, max_seconds, slot_seconds, slots, feed_format)
        self.refresh_s = refresh_s
        self.seg = []                                                   # per batch: u8 [c, L, S] host arrays
        self.emb = []
        self.soft = []                                                  # per batch: f32 [c, L, S] DEVICE tensors (return_scores)
        self.last_refresh_n = 0
        self.stats["refreshes"] = 0

    def _windows(self, res, lo: int, hi: int) -> None:
        self.seg.append(res.segmentations.cpu().numpy())               # 5.7 KB per window
        self.emb.append(res.embeddings.cpu().numpy())
        if self.SCORES:
            self.soft.append(res.scores)

    def feed(self, samples) -> Optional[Annotation]:
        """append float32 samples (16 kHz mono, the pipeline's rate) — or, in a session with a feed_format, bytes / arrays of
        the stored dtype in that format, of any length; returns a provisional annotation when a refresh is due, else None"""
        if self._append(samples) == 0:
            return None
        self._compute(complete_windows(self.n, self.runner.window, self.runner.step))
        if (self.refresh_s is not None and self.done > 0
                and self.n - self.last_refresh_n >= self.refresh_s * self.sr):
            self.last_refresh_n = self.n
            self.stats["refreshes"] += 1
            return self._annotate()
        return None

    def _annotate(self):
        seg, emb = np.concatenate(self.seg), np.concatenate(self.emb)
        if not self.SCORES:
            return self.pipe.host_stage(seg, emb, self.name)
        from .postprocess import crop_end
        chunks = self.pipe.chunks_window()
        grid, _, T = _frame_grid(seg.shape[0], seg.shape[1], chunks, receptive_field(self.sr))
        if self.finished and self._final_windows()[1]:                  # the crop of __call__: the last window was zero-padded
            T = crop_end(T, grid, self.n / self.sr)
        with torch.cuda.device(self.device):
            if len(self.soft) > 1:
                self.soft = [torch.cat(self.soft)]
            return self.pipe.host_stage(seg, emb, self.name, soft=self.soft[0], num_frames=T)

    def finish(self) -> Annotation:
        """end of stream: the zero-padded tail window (if the reference would run one), then the final host stage"""
        if not self.finished:
            self._flush()
        if self.n > 0:
            self._compute(self._final_windows()[0])
        self.finished = True
        if self.done == 0:
            ann = Annotation(uri=self.name)
            if self.SCORES:
                from .core import SlidingWindowFeature
                grid = _frame_grid(0, self.runner.num_frames, self.pipe.chunks_window(), receptive_field(self.sr))[0]
                return ann, SlidingWindowFeature(np.zeros((0, 0), dtype=np.float32), grid)
            return ann
        out = self._annotate()
        self._write_rttm(out[0] if self.SCORES else out)
        return out


def stream(pipeline, chunks: Iterable, sess_name: Optional[str] = None, **kw) -> Iterator[Tuple[float, Annotation]]:
    """generator form: yields (seconds of audio received, provisional Annotation) at every refresh and finally
    (total seconds, final Annotation).  feed_format=audio.FeedFormat(...): the chunks are the source's own bytes.
    return_scores=True: (seconds, Annotation, scores) each time; the final pair is `pipeline(file, return_scores=True)`"""
    sess = StreamingSession(pipeline, sess_name, **kw)
    one = (lambda out: (sess.seconds,) + tuple(out)) if sess.SCORES else (lambda out: (sess.seconds, out))
    for c in chunks:
        ann = sess.feed(c)
        if ann is not None:
            yield one(ann)
    yield one(sess.finish())                                            # (a stored feed: finish() makes the last samples final)


# ----------------------------------------------------------------------------- sessions with a committed prefix
class StreamRows:
    """Growable host rows of a CommittedStream, one named array per output: rows below `frontier` are final, rows below
    `covered` valid (the provisional tail lies between the two).  Needs no device."""

    def __init__(self, **arrays):
        """name = (dtype, trailing shape) per array"""
        self.frontier = 0                                               # rows committed
        self.covered = 0                                                # rows computed (committed + provisional tail)
        self._rows = {k: np.zeros((1024,) + tuple(shape), dtype=dtype) for k, (dtype, shape) in arrays.items()}

    def span(self, upto: int, frontier: int) -> Tuple[int, int, int]:
        """the next step computes rows [t0, t1) = [self.frontier, upto) and commits the rows below `frontier`:
        -> (t0, t1, frontier) with t1 >= t0 and t0 <= frontier <= t1"""
        t0, t1 = self.frontier, max(int(upto), self.frontier)
        return t0, t1, min(max(int(frontier), t0), t1)

    def write(self, t0: int, t1: int, frontier: int, **arrays) -> None:
        """rows [t0, t1) of the named arrays (none when the span is empty), then the new frontier; capacity doubles"""
        for k, a in self._rows.items():
            if t1 > len(a):
                grown = np.zeros((max(t1, 2 * len(a)),) + a.shape[1:], dtype=a.dtype)
                grown[:len(a)] = a
                self._rows[k] = grown
        for k, v in arrays.items():
            self._rows[k][t0:t1] = v
        self.frontier, self.covered = frontier, t1

    def committed(self, name: str) -> np.ndarray:
        """the rows below the frontier (a copy)"""
        return self._rows[name][:self.frontier].copy()

    def valid(self, name: str) -> np.ndarray:
        """the rows below `covered` (a view)"""
        return self._rows[name][:self.covered]


class CommittedStream(WindowStream):
    """A session whose output has a COMMITTED PREFIX: the windows' u8 decisions are kept in one device buffer [cmax, L, S],
    and per feed one range call computes the frames [previous frontier, frames covered so far).

    A frame's result depends only on the windows that cover it, and window start frames do not depend on how many windows
    exist.  With windows 0 .. C - 1 computed, every frame before the start frame of window C (the FRONTIER,
    postprocess.committed_frames) is therefore final: the committed rows are the offline bits and only ever grow.  The frames
    from the frontier to the end of window C - 1 are the provisional tail, which the next window revises — nothing that is
    already final is derived again.

    The subclass gives `_range(t0, t1, frontier)` -> {row name: device tensor [t1 - t0, ...]} and `_annotate()`; it may extend
    `_windows` and `_final_frames`."""

    def __init__(self, pipeline, name: Optional[str], rows: Dict[str, tuple], max_seconds: float = 4 * 3600.0,
                 slot_seconds: float = 10.0, slots: int = 4, feed_format=None, hub=None):
        """rows: the host arrays the range call fills, name -> (dtype, trailing shape) (StreamRows)"""
        dz_dist.require_single_rank(type(self).__name__)
        super().__init__(pipeline, name, max_seconds, slot_seconds, slots, feed_format, hub)
        self.chunks, self.frames = pipeline.chunks_window(), receptive_field(self.sr)
        cmax, L, S = self.ingest.views.shape[0], self.runner.num_frames, pipeline.engine.seg.max_speakers_per_chunk
        self.grid, starts, _ = _frame_grid(cmax, L, self.chunks, self.frames)
        with torch.cuda.device(self.device):
            self.seg = torch.zeros((cmax, L, S), device=self.device, dtype=torch.uint8)     # decisions of every window so far
            self.d_start = torch.from_numpy(starts).to(self.device)
        self.rows = StreamRows(**rows)
        self._last = None
        self.result = None                                              # the final Annotation, once the stream has ended
        self._finish_annotate = None
        self.stats["range_calls"] = 0

    @property
    def frontier(self) -> int:
        """frames committed"""
        return self.rows.frontier

    @property
    def covered(self) -> int:
        """frames computed (committed + provisional tail)"""
        return self.rows.covered

    @property
    def committed_seconds(self) -> float:
        """start time of the first frame that may still change"""
        return self.grid.start + self.frontier * self.grid.step

    def _windows(self, res, lo: int, hi: int) -> None:
        self.seg[lo:hi] = res.segmentations

    def _advance(self, upto_frames: int, frontier: int) -> None:
        """one range call over [self.frontier, upto_frames); frames below `frontier` are committed"""
        t0, t1, frontier = self.rows.span(upto_frames, frontier)
        out = {}
        if t1 > t0:
            out = self._range(t0, t1, frontier)
            self.stats["range_calls"] += 1
        self.rows.write(t0, t1, frontier, **{k: v.cpu().numpy() for k, v in out.items()})

    def _range(self, t0: int, t1: int, frontier: int) -> dict:
        raise NotImplementedError

    def _annotate(self) -> Annotation:
        raise NotImplementedError

    def _final_frames(self, T: int, has_last: bool) -> int:
        """the length of the final output, given the T frames the windows cover"""
        return T

    def feed(self, samples) -> Optional[Annotation]:
        """append float32 samples (mono, the pipeline's rate), or bytes / stored-dtype arrays in the session's feed_format.
        -> None while no window is complete, else the Annotation over
        every frame computed so far (final before `committed_seconds`, provisional after).
        A hub's session: host work only — the feed is staged, the hub's next tick() runs it; -> the latest Annotation"""
        with torch.cuda.device(self.device):
            taken = self._append(samples)
            if self.hub is not None:
                return self._last
            upto = complete_windows(self.n, self.runner.window, self.runner.step)
            if taken and upto > self.done:
                self._compute(upto)
                self._step()
        return self._last

    def _step(self) -> Annotation:
        """the new windows are in: one range call up to the frames they cover, the frontier moves, the annotation follows"""
        self._advance(covered_frames(self.done, self.chunks, self.frames, self.grid),
                      committed_frames(self.done, self.chunks, self.frames, self.grid))
        self._last = self._annotate()
        return self._last

    def finish(self, annotate: Optional[Callable[[], Annotation]] = None) -> Annotation:
        """end of stream: the zero-padded last window if the reference would run one, every frame of the final length
        committed -> `annotate()` (default: `_annotate`), written as RTTM where the subclass's `_write_rttm` says so.
        A hub's session: marks the end of the stream and returns None; the hub's NEXT tick() does all of the above, its result
        holds the final Annotation, which stays in `result`"""
        if self.finished:
            raise RuntimeError("stream already finished")
        if self.hub is not None:
            self.finished, self._finish_annotate = True, annotate
            return None
        with torch.cuda.device(self.device):
            self._flush()
        total, has_last = self._final_windows()
        self.finished = True
        if self.n == 0:
            self.result = Annotation(uri=self.name)
            return self.result
        with torch.cuda.device(self.device):
            self._compute(total)
        return self._finish_end(has_last, annotate)

    def _finish_end(self, has_last: bool, annotate: Optional[Callable[[], Annotation]] = None) -> Annotation:
        """every window is in: commit every frame of the final length -> the final Annotation and its RTTM file"""
        with torch.cuda.device(self.device):
            T = self._final_frames(covered_frames(self.done, self.chunks, self.frames, self.grid), has_last)
            assert self.frontier <= T, "committed frames beyond the offline output"
            self._advance(T, T)
        ann = self._last = self.result = (annotate or self._annotate)()
        self._write_rttm(ann)
        return ann


def stream_committed(sess: CommittedStream, chunks: Iterable, **finish_kw) -> Iterator[Tuple[float, float, Annotation]]:
    """generator form of a CommittedStream: chunks of float32 samples at the pipeline's rate (or of the session's
    feed_format) -> (seconds received, committed
    seconds, Annotation) for every feed that produced an annotation, then the final triple"""
    for c in chunks:
        ann = sess.feed(c)
        if ann is not None:
            yield sess.seconds, sess.committed_seconds, ann
    ann = sess.finish(**finish_kw)
    yield sess.seconds, sess.committed_seconds, ann
