"""A live hub: many concurrent sessions, one batched forward per tick.

    hub = pipeline.open_hub(max_sessions=64, max_seconds=600.0)                 # DiariZenPipeline: LiveDiarization sessions
    hub = VoiceActivityDetection(pipeline).open_hub(max_sessions=64)            # detection pipelines: DetectionStream sessions
    a = hub.open("call-17", feed_format=FeedFormat(8000, "ulaw", channels=2, channel=1))     # keywords of open_live / open_stream
    a.feed(packet)                        # host only: the bytes go to the session's FeedPlanner, nothing touches the device
    out = hub.tick()                      # ALL device work for everything fed since the last tick -> {name: Annotation}
    a.finish()                            # marks the end; the NEXT tick flushes, runs the last window, commits, writes the RTTM
    hub.close()

A box that terminates calls has a few hundred streams, each delivering a 20 ms packet fifty times a second.  Opened one by one
(open_live / open_stream) every session is an island: its own pinned ring, device twins, copy stream and 4 h device buffer, one
H2D copy and one launch-bound dzn_resample per packet, and a whole engine forward — about 180 launches — for a batch of ONE
window whenever it completes one.  Per-window results are batch-invariant and chunking-invariant, so running the windows of
many sessions in one forward changes no bit of any session's output; it only needs an owner that sees all sessions at once.

What one tick() does:
  a. ONE staging upload: the FeedCalls of every session (audio.FeedPlanner, unchanged; float32 feeds are decode calls) are
     packed into one slot of ONE pinned ring — the descriptor table first, then each call's bytes padded to 16 B (`pack_tick`)
     — and one non_blocking H2D moves the slot to its device twin on the hub's copy stream.  A tick whose bytes exceed a slot
     splits into as few uploads as fit; a slot is reused only after the event recorded behind the kernel that read its twin;
  b. ONE ingest launch per upload: dzn_ingest_many (csrc/ingest.hip) decodes and resamples every descriptor's range straight
     into that session's row of ONE pooled, pre-zeroed device buffer f32 [max_sessions, max_seconds * rate + window].  A row
     plays the part of WaveIngest.dev_wave, zeros behind the last sample included; every sample has the bits of the single
     dzn_resample / dzn_decode call;
  c. the batched forward: every window that became complete, over all sessions, oldest first within a session, is copied by
     dzn_gather_windows into dense batches [B, window] of at most batch_size windows, balanced as WindowRunner.run_views
     balances them (`plan_batches`), and runs segment -> prepare_masks -> embed (the dense entry: the same bits as the strided
     one, tests/test_fbank_shared_gpu.py).  ceil(ready / batch_size) forwards per tick, not one per session; the compute
     stream waits for the ingest event only;
  d. ONE D2H of the tick's decisions and embeddings (diarization; detection needs neither on the host), then per session, in
     window order, the host labelling and the session's own range call (dzn_diarize_range / dzn_detect_range) — the sessions
     are ordinary LiveDiarization / DetectionStream objects whose "take results" and "advance" steps the hub calls
     (streaming.WindowStream).  The range calls stay per session; `stats` counts them;
     A session opened with `scores=True` (live.LiveDiarization) makes the tick's forwards write the classifier's soft output as
     well — only in a tick where such a session has new windows — into a device tensor that never goes to the host; the
     session copies its rows device to device and its range call is dzn_diarize_range_scores, still one launch;
  e. `stats`: {"ticks", "tick": the last tick's counters, "total": their sums} with uploads, ingest_launches, forwards,
     windows, range_calls and sessions_advanced.

Memory: max_sessions x (max_seconds x rate + window) x 4 B for the pool — 64 x 600 s is 2.5 GB — plus, per OPEN session, its
decision buffer u8 [windows, L, S] (and int8 [windows, S] labels), about 1.2 MB at 600 s.  The default max_seconds of a hub is
deliberately far below the 4 h of a solo session: the pool is allocated up front for every row.

A finished session's row goes to the next session that opens: the row is zeroed over [0, n_old + window) on the copy stream,
after an event recorded behind the compute stream's last gather from it and before the new session's first ingest write."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import audio as audio_io
from . import dist as dz_dist
from .core import Annotation

DESC_BYTES = 96                             # sizeof(dzn_ingest_desc), include/dzn.h
ARRAY_DESC_BYTES = 208                      # sizeof(dzn_beamform_desc)
ALIGN = 16                                  # every call's bytes start on a 16-byte boundary of the slot
COUNTERS = ("uploads", "ingest_launches", "forwards", "windows", "range_calls", "sessions_advanced", "array_calls",
            "array_launches")
STATE_INTS = 5                              # DZN_BEAMFORM_STATE_INTS
ARRAY_MIN_HOP, ARRAY_MAX_HOP = 256, 4096    # the hops audio.Beamform.plan can give
ARRAY_CALL_HOPS = 4                         # an array call takes at most this many hops of new frames
# the history a resample range still reads is shorter than K = 2 width + o, and a ratio the hub admits stages one tile's input
# — more than K floats — in the resampler's 64 KiB of LDS (audio.resample_tile_fits): K < 16384 for every admitted feed
ARRAY_HISTORY = 16384


def _pad(nbytes: int) -> int:
    return -(-int(nbytes) // ALIGN) * ALIGN


# ----------------------------------------------------------------------------- host: packing and scheduling
class Upload:
    """one slot's image: `desc` the descriptor table (records of _lib.ingest_desc_dtype(), src_offset and tile0 filled in),
    `chunks` = [(byte offset in the slot, bytes)] behind it, `nbytes` the bytes to copy, `tiles` the table's tile total,
    `keys` the owner of every descriptor (what the caller passed) and `sizes` the bytes of its call"""
    __slots__ = ("desc", "chunks", "nbytes", "tiles", "keys", "sizes")

    def __init__(self, desc, chunks, nbytes, tiles, keys, sizes):
        self.desc, self.chunks, self.nbytes, self.tiles, self.keys, self.sizes = desc, chunks, nbytes, tiles, keys, sizes

    def image(self) -> np.ndarray:
        """the slot's first nbytes as they are uploaded"""
        out = np.zeros(self.nbytes, dtype=np.uint8)
        out[:len(self.desc) * DESC_BYTES] = self.desc.view(np.uint8)
        for off, data in self.chunks:
            out[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        return out


def pack_tick(calls: Sequence[Tuple[object, dict, bytes]], slot_bytes: int, tile: int) -> List[Upload]:
    """calls: (key, descriptor fields but src_offset / tile0, the call's bytes) in the order they were planned -> the uploads
    of one tick, as few as fit and in the same order (a session's calls are never reordered): per slot the table of its
    descriptors, then each call's bytes at a 16-byte boundary.  tile0 is the tile prefix INSIDE an upload (one launch each);
    a descriptor with m1 = m0 owns no tile."""
    dt = _lib.ingest_desc_dtype()
    groups, cur, used = [], [], 0
    for call in calls:
        need = DESC_BYTES + _pad(len(call[2]))
        if need > slot_bytes:
            raise ValueError(f"a call of {len(call[2])} bytes does not fit a staging slot of {slot_bytes} bytes")
        if cur and used + need > slot_bytes:
            groups.append(cur)
            cur, used = [], 0
        cur.append(call)
        used += need
    if cur:
        groups.append(cur)
    ups = []
    for g in groups:
        desc = np.zeros(len(g), dtype=dt)
        for k in set().union(*(c[1] for c in g)):                           # column by column: a tick of 64 calls is 13 assignments
            desc[k] = [c[1].get(k, 0) for c in g]
        off, tiles, chunks, offs, tile0 = len(g) * DESC_BYTES, 0, [], [], []
        for _, fields, data in g:
            offs.append(off)
            tile0.append(tiles)
            if len(data):
                chunks.append((off, data))
            off += _pad(len(data))
            tiles += -(-(int(fields["m1"]) - int(fields["m0"])) // tile)
        desc["src_offset"], desc["tile0"] = offs, tile0
        ups.append(Upload(desc, chunks, off, tiles, [c[0] for c in g], [len(c[2]) for c in g]))
    return ups


class ArrayUpload:
    """one slot's image of an array wave: `desc` the table of _lib.beamform_desc_dtype() records, `chunks` = [(byte offset in
    the slot, bytes)] behind it, `rdesc` the dzn_ingest_desc records of the calls that resample (their staging buffer is the
    beamformed staging pool) at byte `roff` of the slot, `nbytes` the bytes to copy, `keys` the owner of every descriptor and
    `calls` its planned call"""
    __slots__ = ("desc", "chunks", "rdesc", "roff", "nbytes", "keys", "calls")

    def __init__(self, desc, chunks, rdesc, roff, nbytes, keys, calls):
        self.desc, self.chunks, self.rdesc, self.roff, self.nbytes = desc, chunks, rdesc, roff, nbytes
        self.keys, self.calls = keys, calls

    def image(self) -> np.ndarray:
        """the slot's first nbytes as they are uploaded"""
        out = np.zeros(self.nbytes, dtype=np.uint8)
        out[:len(self.desc) * ARRAY_DESC_BYTES] = self.desc.view(np.uint8)
        for off, data in self.chunks:
            out[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        if len(self.rdesc):
            out[self.roff:self.roff + len(self.rdesc) * DESC_BYTES] = self.rdesc.view(np.uint8)
        return out


def array_waves(queue: Sequence[tuple]) -> List[list]:
    """queue: (key, ...) entries in the order they were planned -> waves: wave j holds the j-th entry of every key, in queue
    order.  Two calls of one session never share a wave (the second reads the tracker state the first writes and the staging
    buffer it fills), a session's calls stay in order over the waves, and every entry appears exactly once."""
    waves, count = [], {}
    for entry in queue:
        j = count.get(entry[0], 0)
        count[entry[0]] = j + 1
        if j == len(waves):
            waves.append([])
        waves[j].append(entry)
    return waves


def pack_array_waves(calls: Sequence[tuple], slot_bytes: int, tile: int, beam_tile: int, planar_floats: int,
                     temp_elems: int) -> List[ArrayUpload]:
    """calls: (key, the call, its dzn_beamform_desc fields but src_offset / planar_offset / lag_offset / the three prefixes,
    its dzn_ingest_desc fields but tile0 when it resamples else None, its bytes) in the order they were planned -> the uploads
    of one tick: the waves of `array_waves`, each split in order where it exceeds a slot or the shared scratch.  Per slot: the
    descriptor table, each call's bytes at a 16-byte boundary, then the resample descriptors.  A descriptor owns
    ceil(src_frames / beam_tile) decode tiles, (b1 - b0) (channels - 1) GCC-PHAT work items and ceil((n1 - s_first) /
    beam_tile) sum tiles; its planar decode [channels][src_frames] and lag / peak rows [channels][b1 - b0] lie one behind the
    other in the scratch."""
    dt, rdt = _lib.beamform_desc_dtype(), _lib.ingest_desc_dtype()
    groups = []
    for wave in array_waves(calls):
        cur, used, planar, temp = [], 0, 0, 0
        for entry in wave:
            _, _, f, res, data = entry
            need = ARRAY_DESC_BYTES + _pad(len(data)) + (DESC_BYTES if res is not None else 0)
            pl, tm = int(f["channels"]) * int(f["src_frames"]), int(f["channels"]) * (int(f["b1"]) - int(f["b0"]))
            if need > slot_bytes or pl > planar_floats or tm > temp_elems:
                raise ValueError(f"an array call of {len(data)} bytes does not fit a staging slot of {slot_bytes} bytes")
            if cur and (used + need > slot_bytes or planar + pl > planar_floats or temp + tm > temp_elems):
                groups.append(cur)
                cur, used, planar, temp = [], 0, 0, 0
            cur.append(entry)
            used, planar, temp = used + need, planar + pl, temp + tm
        if cur:
            groups.append(cur)
    ups = []
    for g in groups:
        desc = np.zeros(len(g), dtype=dt)
        for k in set().union(*(e[2] for e in g)):
            desc[k] = [e[2].get(k, 0) for e in g]
        off, chunks = len(g) * ARRAY_DESC_BYTES, []
        planar = temp = dtiles = items = stiles = 0
        for i, (_, _, f, _, data) in enumerate(g):
            C_, frames, nblk = int(f["channels"]), int(f["src_frames"]), int(f["b1"]) - int(f["b0"])
            desc[i]["src_offset"], desc[i]["planar_offset"], desc[i]["lag_offset"] = off, planar, temp
            desc[i]["decode_tile0"], desc[i]["gcc_item0"], desc[i]["sum_tile0"] = dtiles, items, stiles
            if len(data):
                chunks.append((off, data))
            off += _pad(len(data))
            planar, temp = planar + C_ * frames, temp + C_ * nblk
            dtiles += -(-frames // beam_tile)
            items += nblk * (C_ - 1)
            stiles += -(-(int(f["n1"]) - int(f["s_first"])) // beam_tile)
        res = [e[3] for e in g if e[3] is not None]
        rdesc = np.zeros(len(res), dtype=rdt)
        if res:
            for k in set().union(*res):
                rdesc[k] = [r.get(k, 0) for r in res]
            counts = [-(-(int(r["m1"]) - int(r["m0"])) // tile) for r in res]
            rdesc["tile0"] = np.cumsum([0] + counts[:-1])
        ups.append(ArrayUpload(desc, chunks, rdesc, off, off + len(res) * DESC_BYTES, [e[0] for e in g], [e[1] for e in g]))
    return ups


def plan_batches(ready: Sequence[int], batch_size: int) -> List[List[Tuple[int, int]]]:
    """ready[i]: new complete windows of session i -> the tick's forwards: lists of (session index, k-th new window of that
    session), every ready window exactly once, sessions in order and oldest first within a session, ceil(total / batch_size)
    batches of (almost) equal size — the balance of WindowRunner.run_views.  Nothing ready: no forward."""
    flat = [(i, k) for i, c in enumerate(ready) for k in range(int(c))]
    if not flat:
        return []
    nb = -(-len(flat) // int(batch_size))
    bs = -(-len(flat) // nb)
    return [flat[b:b + bs] for b in range(0, len(flat), bs)]


class RowFeed:
    """The host half of a hub session's ingest, with WaveIngest's counters: feeds become planned calls in the book's queue
    (`append` / `flush` touch no device), the hub's tick moves them to the device and then advances `n`.  The hub attaches the
    device half: `dev_wave` (the session's pool row) and `views` (its windows)."""

    def __init__(self, book: "HubBook", row: int, plan):
        self.book, self.row, self.plan = book, row, plan
        self.sr, self.window, self.capacity = book.sr, book.window, book.row_floats
        self.n = 0                          # model-rate samples on the device (after the tick that ingested them)
        self.staged = 0                     # ... including the calls still queued
        self.frames = 0                     # source frames received
        self.uploads = 0                    # planned calls that went to the device
        self.ended = False
        self.dev_wave = self.views = None
        self._wait = None
        # an array row (plan: audio.ArrayFeedPlanner).  `seen` is the host's count of blocks tracked on the row's device state
        # (advanced by the hub behind a successful dzn_beamform_many), `planned` the same count over the calls whose
        # descriptors have been written; stage_at / stage_first: the staging buffer that will hold the beamformed samples
        # stage_first .. once those calls have run
        self.array = isinstance(plan, audio_io.ArrayFeedPlanner)
        self.seen = self.planned = 0
        self.stage_at = self.stage_first = 0
        self._delays = None

    def _refuse_longer(self, length: int) -> None:
        if length + self.window > self.capacity:
            raise MemoryError(f"stream longer than max_seconds = {(self.capacity - self.window) / self.sr:.0f} s")

    def append(self, samples) -> int:
        """-> model-rate samples staged (float32 feed: samples taken)"""
        if self.ended:
            raise RuntimeError("stream already finished")
        if self.plan is not None:
            data = audio_io._feed_bytes(samples, self.plan.fmt)
            self._refuse_longer(self.plan.length_after(len(data)))
            staged = self._queue(self.plan.append(data))
            self.frames = self.plan.frames
            return staged
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float32).reshape(-1))
        self._refuse_longer(self.staged + len(x))
        per = self.book.max_call_bytes // 4
        calls, m = [], self.staged
        for a in range(0, len(x), per):
            k = min(per, len(x) - a)
            calls.append(audio_io.FeedCall(x[a:a + k].tobytes(), m, k, m + k, m, m + k))
            m += k
        self.frames = m
        return self._queue(calls)

    def flush(self) -> int:
        """end of stream: the samples of a stored feed that waited for frames which will not come"""
        self.ended = True
        return 0 if self.plan is None else self._queue(self.plan.finish())

    def _queue(self, calls) -> int:
        s0 = self.staged
        for c in calls:
            assert c.m0 == self.staged and c.m1 + self.window <= self.capacity
            self.book.queue.append((self, c))
            self.staged = c.m1
        return self.staged - s0

    def fields(self, c) -> dict:
        """the descriptor of planned call c (but src_offset / tile0, which the packer writes)"""
        base = self.row * self.capacity + c.m0
        if self.plan is None:
            return dict(src_format=0, channels=1, channel=0, src_first_index=c.first, src_len=c.frames, total_len=c.total,
                        m0=c.m0, m1=c.m1, bank_offset=-1, dst_offset=base, o=1, n=1, width=0)
        p, f = self.plan, self.plan.fmt
        return dict(src_format=f.src_format, channels=f.channels, channel=f.channel_code(), src_first_index=c.first,
                    src_len=c.frames, total_len=c.total, m0=c.m0, m1=c.m1,
                    bank_offset=-1 if p.same_rate else self.book.bank_offset(f.rate), dst_offset=base,
                    o=p.o, n=p.n, width=p.width)

    def array_fields(self, c) -> Tuple[dict, Optional[dict]]:
        """planned array call c (an audio.ArrayFeedCall; called once per call, in order) -> its dzn_beamform_desc fields but
        what the packer writes, and the dzn_ingest_desc fields (but tile0) of the resampling behind it, or None.  A feed at
        the model's rate sums straight into the pool row.  Otherwise the call fills the staging buffer the call before did
        NOT fill: [s_first, n0) is carried over from that one (WaveIngest._run_array copies it device to device), [n0, n1) is
        made, and the resampler reads [s_first, n1) — the arguments _run_array gives dzn_resample."""
        p, f, b = self.plan, self.plan.fmt, self.book
        d = dict(src_format=f.src_format, channels=f.channels, src_first=c.first, src_frames=c.frames, T=c.total,
                 ref=p.beamform.reference, hop=p.hop, max_lag=p.max_lag, min_peak=p.min_peak,
                 twiddle_offset=b.twiddle_offset(p.hop), ch_stride=c.frames, blk_cap=c.b1 - c.b0, b0=c.b0, b1=c.b1,
                 seen=self.planned, state_offset=self.row * b.array_channels * STATE_INTS,
                 delay_offset=self.row * b.array_channels * b.table_blocks, table_blocks=b.table_blocks, n0=c.n0, n1=c.n1)
        assert c.b1 <= b.table_blocks
        self.planned = c.b1
        res = None
        if p.same_rate:
            d.update(s_first=c.n0, dst_space=0, dst_offset=self.row * self.capacity + c.n0, carry_offset=-1)
        elif c.n1 > c.n0 or c.m1 > c.m0:
            old, new = self.stage_at, self.stage_at ^ 1
            hist = c.n0 - c.s_first                                     # < K beamformed samples a later range still reads
            assert c.s_first >= self.stage_first and hist + c.n1 - c.n0 <= b.stage_floats
            at = b.stage_offset(self.row, new)
            d.update(s_first=c.s_first, dst_space=1, dst_offset=at,
                     carry_offset=b.stage_offset(self.row, old) + c.s_first - self.stage_first if hist else -1)
            self.stage_at, self.stage_first = new, c.s_first
            if c.m1 > c.m0:
                res = dict(src_offset=4 * at, src_format=0, channels=1, channel=0, src_first_index=c.s_first,
                           src_len=c.n1 - c.s_first, total_len=c.n1, m0=c.m0, m1=c.m1, bank_offset=b.bank_offset(f.rate),
                           dst_offset=self.row * self.capacity + c.m0, o=p.o, n=p.n, width=p.width)
        else:                                                           # blocks only: nothing is summed, nothing carried
            d.update(s_first=c.n0, dst_space=1, dst_offset=b.stage_offset(self.row, self.stage_at ^ 1), carry_offset=-1)
        return d, res

    def delays(self) -> np.ndarray:
        """int32 [C, blocks]: the row's delay table as far as the device has filled it (after the tick behind finish(): of the
        whole recording).  The one call that waits for the device."""
        if not self.array or self._delays is None:
            raise ValueError("delays(): not an array feed")
        return self._delays(self)

    def wait(self) -> None:
        """the current (compute) stream runs behind the newest ingest launch"""
        if self._wait is not None:
            self._wait()


class HubBook:
    """The host bookkeeping of a hub, no device: who is open and in which row, what is refused, and the queue of planned calls
    since the last tick."""

    def __init__(self, max_sessions: int, max_seconds: float, sample_rate: int, window: int, step: int, slot_bytes: int,
                 tile: int, array_channels: int = 0, array_rate: Optional[int] = None, beam_tile: int = 1024):
        """array_channels / array_rate: the most microphones and the highest feed rate of an array session (0: the hub
        takes no array feeds); beam_tile: dzn_beamform_tile()"""
        if isinstance(max_sessions, bool) or int(max_sessions) != max_sessions or max_sessions < 1:
            raise ValueError(f"max_sessions is a positive integer, not {max_sessions!r}")
        if not max_seconds > 0:
            raise ValueError(f"max_seconds is a positive number of seconds, not {max_seconds!r}")
        self.max_sessions, self.max_seconds = int(max_sessions), float(max_seconds)
        self.sr, self.window, self.step, self.tile = int(sample_rate), int(window), int(step), int(tile)
        self.row_floats = int(max_seconds * self.sr) + self.window           # + one window of zeros behind the last sample
        self.slot_bytes = int(slot_bytes)
        self.max_call_bytes = (self.slot_bytes - DESC_BYTES) // ALIGN * ALIGN
        if self.max_call_bytes < 4 * ALIGN:
            raise ValueError(f"slot_bytes = {slot_bytes} holds no call")
        self.names: Dict[str, int] = {}                                     # open sessions -> row
        self.free = list(range(self.max_sessions))
        self.queue: list = []                                               # (RowFeed, FeedCall) since the last tick
        self.bank_offsets: Dict[int, int] = {}                              # feed rate -> float offset of its bank (the hub fills it)
        self.new_bank: Optional[Callable[[int], int]] = None
        if (isinstance(array_channels, bool) or not isinstance(array_channels, (int, np.integer))
                or not (array_channels == 0 or 2 <= array_channels <= 64)):
            raise ValueError(f"array_channels is 0 (no array feeds) or an integer in [2, 64], not {array_channels!r}")
        if array_rate is not None:
            if not array_channels:
                raise ValueError("array_rate needs array_channels: a hub opened with array_channels=0 takes no array feeds")
            if isinstance(array_rate, bool) or not isinstance(array_rate, (int, np.integer)) or array_rate < 1:
                raise ValueError(f"array_rate is a positive integer, not {array_rate!r}")
        self.array_channels, self.beam_tile = int(array_channels), int(beam_tile)
        self.array_rate = (self.sr if array_rate is None else int(array_rate)) if self.array_channels else 0
        self.array_max_call_bytes = (self.slot_bytes - ARRAY_DESC_BYTES - DESC_BYTES) // ALIGN * ALIGN
        # the delay table of a row: the blocks of max_seconds at array_rate with the smallest hop
        self.table_blocks = -(-(int(self.max_seconds * self.array_rate) + 1) // ARRAY_MIN_HOP) + 2 if self.array_channels else 0
        self.stage_floats = ARRAY_HISTORY + ARRAY_CALL_HOPS * ARRAY_MAX_HOP     # one of a row's two beamformed staging buffers
        # scratch shared by the calls of one wave: a stored sample is at least a byte, so the planar decodes of the calls in a
        # slot are at most slot_bytes floats; a call completes at most frames / hop + 1 blocks (+ the two last ones at the
        # end), channels x that is below bytes / 256 + its own descriptor's 208
        self.planar_floats = self.temp_elems = self.slot_bytes if self.array_channels else 0
        self.twiddle_offsets: Dict[int, int] = {}                           # hop -> float offset of its twiddle table
        self.new_twiddle: Optional[Callable[[int], int]] = None

    def bank_offset(self, rate: int) -> int:
        if rate not in self.bank_offsets:
            self.bank_offsets[rate] = self.new_bank(rate)
        return self.bank_offsets[rate]

    def twiddle_offset(self, hop: int) -> int:
        if hop not in self.twiddle_offsets:
            self.twiddle_offsets[hop] = self.new_twiddle(hop)
        return self.twiddle_offsets[hop]

    def stage_offset(self, row: int, which: int) -> int:
        """float offset of staging buffer `which` (0 / 1) of `row` in the pool of beamformed staging buffers"""
        return (2 * row + which) * self.stage_floats

    def array_memory(self) -> Dict[str, int]:
        """bytes of what a hub allocates for array feeds: per-row state, delay tables and staging buffers, shared scratch"""
        rows, ch = self.max_sessions, self.array_channels
        if not ch:
            return dict(state=0, delay=0, staging=0, scratch=0)
        return dict(state=4 * rows * ch * STATE_INTS, delay=4 * rows * ch * self.table_blocks,
                    staging=4 * rows * 2 * self.stage_floats, scratch=4 * (self.planar_floats + 2 * self.temp_elems))

    def _admit_array(self, fmt):
        """the planner of an array feed, or its refusal by name"""
        from .streaming import plan_feed
        if not fmt.channel.causal:
            raise ValueError(f"FeedFormat: channel={fmt.channel!r} is not causal, and a live feed cannot look at later blocks: "
                             "pass Beamform(causal=True)")
        if fmt.channels > self.array_channels:
            raise ValueError(f"feed_format: {fmt!r} has {fmt.channels} channels, and this hub was opened with array_channels = "
                             f"{self.array_channels}")
        if fmt.rate > self.array_rate:
            raise ValueError(f"feed_format: {fmt!r} is at {fmt.rate} Hz, and this hub was opened with array_rate = "
                             f"{self.array_rate}")
        hop, max_lag, _ = fmt.channel.plan(fmt.rate, fmt.channels)
        room = self.array_max_call_bytes // fmt.frame_bytes - 2 * hop - max_lag
        if room < 1:
            raise ValueError(f"feed_format: {fmt!r} needs {(2 * hop + max_lag + 1) * fmt.frame_bytes} bytes per call (two hops "
                             f"of {hop} frames, the search range and one new frame), a staging slot holds "
                             f"{self.array_max_call_bytes}: open the hub with a larger slot_bytes")
        plan = plan_feed(fmt, self.sr, min(room, ARRAY_CALL_HOPS * hop), self.tile)
        assert plan.max_new <= ARRAY_CALL_HOPS * ARRAY_MAX_HOP and (plan.same_rate or plan.K <= ARRAY_HISTORY)
        return plan

    def check_open(self, name) -> None:
        """the refusals of open() that concern the hub, by name"""
        if not isinstance(name, str) or not name:
            raise ValueError(f"a hub session needs a name (a non-empty str), not {name!r}")
        if name in self.names:
            raise ValueError(f"a session named {name!r} is already open in this hub")
        if not self.free:
            raise RuntimeError(f"the hub is full: max_sessions = {self.max_sessions} sessions are open")

    def admit(self, feed_format) -> RowFeed:
        """a row for a new session, or the refusal of a feed_format the device ingest cannot serve (as WaveIngest refuses
        it), before anything is taken"""
        from .streaming import plan_feed
        plan = None
        if feed_format is not None:
            if not isinstance(feed_format, audio_io.FeedFormat) or feed_format.channel is None:
                raise ValueError(f"feed_format is an audio.FeedFormat with a channel choice, not {feed_format!r}")
            if isinstance(feed_format.channel, audio_io.Beamform) and not self.array_channels:
                raise ValueError(f"feed_format: {feed_format!r} is an array feed (channel=Beamform): a hub's rows share one "
                                 "batched ingest launch, which does not beamform; open the session on its own (open_live / "
                                 "open_stream / pipeline.stream)")
            if isinstance(feed_format.channel, audio_io.Beamform):
                plan = self._admit_array(feed_format)
            else:
                hist = 0
                if feed_format.rate != self.sr:
                    o, _, width = audio_io.resample_ratio(feed_format.rate, self.sr)
                    hist = 2 * width + o - 1
                slot_frames = self.max_call_bytes // feed_format.frame_bytes - hist
                if slot_frames < 1:
                    raise ValueError(f"feed_format: {feed_format!r} needs {(hist + 1) * feed_format.frame_bytes} bytes per call, "
                                     f"a staging slot holds {self.max_call_bytes}")
                plan = plan_feed(feed_format, self.sr, slot_frames, self.tile)
        if not self.free:
            raise RuntimeError(f"the hub is full: max_sessions = {self.max_sessions} sessions are open")
        return RowFeed(self, self.free.pop(0), plan)

    def release(self, name: str, row: int) -> None:
        del self.names[name]
        self.free.append(row)

    def take_queue(self) -> list:
        """-> [(RowFeed, FeedCall, its descriptor fields, its bytes)] of everything planned since the last tick by the
        ordinary rows, in order; the array rows' calls stay for `take_array_queue`"""
        q = [(feed, c) for feed, c in self.queue if not feed.array]
        self.queue = [(feed, c) for feed, c in self.queue if feed.array]
        return [(feed, c, feed.fields(c), c.data) for feed, c in q]

    def take_array_queue(self) -> list:
        """-> [(RowFeed, ArrayFeedCall, its dzn_beamform_desc fields, its resample fields or None, its bytes)] of everything
        planned since the last tick by the array rows, in order"""
        q = [(feed, c) for feed, c in self.queue if feed.array]
        self.queue = [(feed, c) for feed, c in self.queue if not feed.array]
        return [(feed, c, *feed.array_fields(c), c.data) for feed, c in q]


class _TickResult:
    """what a session takes from a tick's forwards: its new windows' rows of the device results, and of the host copy;
    `scores`: their rows of the tick's soft scores (device; None in a tick where no ready session asked for them)"""
    __slots__ = ("segmentations", "embeddings", "host", "scores")

    def __init__(self, segmentations, embeddings, host, scores=None):
        self.segmentations, self.embeddings, self.host, self.scores = segmentations, embeddings, host, scores


# ----------------------------------------------------------------------------- the hub
class LiveHub:
    def __init__(self, pipeline, make_session: Callable, max_sessions: int = 64, max_seconds: float = 600.0,
                 slot_bytes: int = 1 << 20, slots: int = 4, array_channels: int = 0, array_rate: Optional[int] = None):
        """pipeline: a DiariZenPipeline or a detection pipeline (its _runner and device are used); make_session(name, hub,
        **kw) -> the CommittedStream of a new session; max_sessions x max_seconds size the pooled device buffer, slot_bytes
        x slots the pinned staging ring and its device twins; array_channels > 0: the hub takes array feeds of at most that
        many microphones at up to array_rate Hz (default: the model's rate) and allocates their tables and scratch here"""
        import torch
        dz_dist.require_single_rank(type(self).__name__)
        self.pipe, self._make = pipeline, make_session
        self.runner = r = pipeline._runner
        self.device = torch.device(pipeline.device)
        self.book = HubBook(max_sessions, max_seconds, r.sample_rate, r.window, r.step, slot_bytes, audio_io.resample_tile(),
                            array_channels, array_rate, audio_io.beamform_tile() if array_channels else 1024)
        self.book.new_bank = self._new_bank
        self.book.new_twiddle = self._new_twiddle
        self.sessions: Dict[str, object] = {}
        self._pending_row = None
        self.closed = False
        b = self.book
        with torch.cuda.device(self.device):
            self.pool = torch.zeros((b.max_sessions, b.row_floats), device=self.device, dtype=torch.float32)
            self.ring = [torch.empty(b.slot_bytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self.ring_np = [t.numpy() for t in self.ring]
            self.twins = [torch.empty(b.slot_bytes, device=self.device, dtype=torch.uint8) for _ in range(slots)]
            self.dense = torch.empty((r.batch_size, r.window), device=self.device, dtype=torch.float32)
            self.arrays = None
            if b.array_channels:                                            # everything an array feed needs, once
                rows, ch, i32, f32 = b.max_sessions, b.array_channels, torch.int32, torch.float32
                self.arrays = dict(state=torch.zeros(rows * ch * STATE_INTS, device=self.device, dtype=i32),
                                   delay=torch.zeros(rows * ch * b.table_blocks, device=self.device, dtype=i32),
                                   beam=torch.zeros(rows * 2 * b.stage_floats, device=self.device, dtype=f32),
                                   planar=torch.empty(b.planar_floats, device=self.device, dtype=f32),
                                   lag=torch.empty(b.temp_elems, device=self.device, dtype=i32),
                                   peak=torch.empty(b.temp_elems, device=self.device, dtype=f32))
            self.copy_stream = torch.cuda.Stream(device=self.device)
            # the pool's zero fill is queued on the current stream, the ingest runs on copy_stream (WaveIngest has the same edge)
            self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
            for t in [self.pool] + self.twins + list((self.arrays or {}).values()):
                t.record_stream(self.copy_stream)
        self.twiddles = None                                                # f32: every hop's twiddle table, one behind the other
        self.banks = None                                                   # f32: every feed rate's bank, one behind the other
        self.slot_free = [None] * slots                                     # event behind the kernel that read the slot's twin
        self.next_slot = 0
        self.ingest_event = None
        self._gathered = None                                               # event behind the newest tick's last gather
        self.row_dirty: Dict[int, tuple] = {}                               # row -> (samples to zero, event behind its last gather)
        self.stats = {"ticks": 0, "tick": dict.fromkeys(COUNTERS, 0), "total": dict.fromkeys(COUNTERS, 0)}

    # ------------------------------------------------------------------ sessions
    def open(self, name: str, **kw):
        """a new session in a free row: the keywords of pipeline.open_live / open_stream but the ingest's (max_seconds,
        slot_seconds, slots are the hub's).  Refused by name, before anything is allocated: a duplicate name, a full hub, a bad
        feed_format, a resample ratio whose tile does not fit LDS, torch.distributed with more than one rank."""
        if self.closed:
            raise RuntimeError("the hub is closed")
        for k in ("max_seconds", "slot_seconds", "slots", "hub"):
            if k in kw:
                raise TypeError(f"open() takes no {k}: the hub's own pool and staging ring hold")
        self.book.check_open(name)
        self._pending_row = None
        try:
            sess = self._make(name, self, **kw)
        except BaseException:
            if self._pending_row is not None:                               # the constructor failed behind the row: give it back
                self.book.free.insert(0, self._pending_row)
            raise
        finally:
            self._pending_row = None
        self.book.names[name] = sess.ingest.row
        self.sessions[name] = sess
        return sess

    def _row_ingest(self, feed_format) -> RowFeed:
        """called by the session's constructor (streaming.WindowStream): refuse, or take a row and prepare it"""
        import torch
        feed = self.book.admit(feed_format)
        row = self._pending_row = feed.row
        with torch.cuda.device(self.device):
            dirty = self.row_dirty.pop(row, None)
            if dirty is not None:                                           # the row's last session: zero what it wrote
                count, gathered = dirty
                with torch.cuda.stream(self.copy_stream):
                    if gathered is not None:
                        self.copy_stream.wait_event(gathered)               # behind the compute stream's last gather from the row
                    self.pool[row, :min(count + self.book.window, self.book.row_floats)].zero_()
            if feed.array:                                                  # a new array session: its tracker starts from zeros
                b = self.book
                with torch.cuda.stream(self.copy_stream):
                    n = b.array_channels * STATE_INTS
                    self.arrays["state"][row * n:(row + 1) * n].zero_()
                    n = b.array_channels * b.table_blocks
                    self.arrays["delay"][row * n:(row + 1) * n].zero_()
                feed._delays = self._row_delays
            feed.dev_wave = self.pool[row]
            feed.views = torch.as_strided(feed.dev_wave, ((feed.capacity - feed.window) // self.book.step + 1, feed.window),
                                          (self.book.step, 1))
        feed._wait = self._wait_ingest
        return feed

    def _wait_ingest(self) -> None:
        import torch
        if self.ingest_event is not None:
            torch.cuda.current_stream(self.device).wait_event(self.ingest_event)

    def _new_bank(self, rate: int) -> int:
        """append the bank of `rate` to the buffer of banks (on copy_stream: behind every launch that reads the old buffer)
        -> its float offset"""
        import torch
        bank = audio_io._device_bank(rate, self.book.sr, self.device)[0].reshape(-1)
        with torch.cuda.stream(self.copy_stream):
            off = 0 if self.banks is None else self.banks.numel()
            self.banks = bank.clone() if self.banks is None else torch.cat([self.banks, bank])
        return off

    def _new_twiddle(self, hop: int) -> int:
        """append the twiddle table of `hop` to the buffer of tables (on copy_stream, as `_new_bank`) -> its float offset"""
        import torch
        tw = torch.from_numpy(audio_io.beamform_twiddle(hop).reshape(-1))
        with torch.cuda.stream(self.copy_stream):
            tw = tw.to(self.device)
            off = 0 if self.twiddles is None else self.twiddles.numel()
            self.twiddles = tw if self.twiddles is None else torch.cat([self.twiddles, tw])
            self.twiddles.record_stream(self.copy_stream)
        return off

    def _row_delays(self, feed: RowFeed) -> np.ndarray:
        b = self.book
        self.copy_stream.synchronize()
        n = b.array_channels * b.table_blocks
        table = self.arrays["delay"][feed.row * n:(feed.row + 1) * n].view(b.array_channels, b.table_blocks)
        return table[:feed.plan.fmt.channels, :feed.seen].cpu().numpy()

    # ------------------------------------------------------------------ the tick
    def tick(self) -> Dict[str, Annotation]:
        """all device work for everything fed (or finished) since the last tick -> {name: Annotation} of the sessions that
        advanced: the annotation over every frame computed so far, or the final one of a session that ended"""
        import torch
        if self.closed:
            raise RuntimeError("the hub is closed")
        t = dict.fromkeys(COUNTERS, 0)
        out: Dict[str, Annotation] = {}
        win, step, b = self.book.window, self.book.step, self.book
        with torch.cuda.device(self.device):
            ending = [s for s in self.sessions.values() if s.finished]
            for s in ending:
                s._flush()                                                  # host: the planner's last call joins the queue
            # a + b: the uploads and their ingest launches
            queued = self.book.take_queue()
            for up in pack_tick([(feed, fields, data) for feed, _, fields, data in queued], self.book.slot_bytes, self.book.tile):
                self._upload(up, t)
            for feed, c, _, _ in queued:
                feed.n = c.m1
                feed.uploads += 1
            # a + b for the array rows: per wave one upload, one dzn_beamform_many, one dzn_ingest_many where a call resamples
            if b.array_channels:
                arrays = b.take_array_queue()
                for up in pack_array_waves(arrays, b.slot_bytes, b.tile, b.beam_tile, b.planar_floats, b.temp_elems):
                    self._upload_wave(up, t)
            for s in self.sessions.values():
                s.stats["uploads"] = s.ingest.uploads
            # c: the windows that became complete
            sessions = list(self.sessions.values())
            upto = []
            for s in sessions:
                if s.finished:
                    upto.append(s._final_windows()[0] if s.n > 0 else 0)
                else:
                    upto.append((0 if s.n < win else (s.n - win) // step + 1))
            ready = [max(u - s.done, 0) for s, u in zip(sessions, upto)]
            batches = plan_batches(ready, self.runner.batch_size)
            total = sum(ready)
            host = seg_all = emb_all = soft_all = None
            if total:
                want_emb = any(s.EMBEDDINGS for s in sessions)
                # the classifier's soft output only in a tick where a session WITH new windows keeps scores; it stays on the device
                want_soft = any(s.SCORES and c for s, c in zip(sessions, ready))
                seg_all, emb_all, buf, soft_all = self._forward(sessions, batches, total, want_emb, t, want_soft)
                if want_emb:                                                # d: ONE D2H of the tick's embeddings and decisions
                    h = buf.cpu().numpy()
                    ne = emb_all.numel() * 4
                    host = (h[ne:].reshape(seg_all.shape), h[:ne].view(np.float32).reshape(emb_all.shape))
            # d (host) + the per-session range calls
            a = 0
            for s, u, c in zip(sessions, upto, ready):
                calls0 = s.stats["range_calls"]
                if c:
                    s._take(_TickResult(seg_all[a:a + c], None if emb_all is None else emb_all[a:a + c],
                                        None if host is None else (host[0][a:a + c].copy(), host[1][a:a + c].copy()),
                                        soft_all[a:a + c] if s.SCORES else None), u)
                    a += c
                if s.finished:
                    if s.n == 0:
                        s.result = s._last = Annotation(uri=s.name)
                    else:
                        s._finish_end(s._final_windows()[1], s._finish_annotate)
                    out[s.name] = s.result
                    self._release(s)
                elif c:
                    out[s.name] = s._step()
                if c or s.finished:
                    t["sessions_advanced"] += 1
                t["range_calls"] += s.stats["range_calls"] - calls0
        t["windows"] = total
        self.stats["ticks"] += 1
        self.stats["tick"] = t
        for k in COUNTERS:
            self.stats["total"][k] += t[k]
        return out

    def _upload(self, up: Upload, t: dict) -> None:
        """one slot: its image to the pinned slot, ONE H2D to the twin, ONE dzn_ingest_many, the slot's event"""
        import torch
        b = self.book
        i = self.next_slot
        if self.slot_free[i] is not None:
            self.slot_free[i].synchronize()                                 # ring full: wait for the oldest copy and its kernel
        slot = self.ring_np[i]
        nd = len(up.desc)
        slot[:nd * DESC_BYTES] = up.desc.view(np.uint8)
        for off, data in up.chunks:
            slot[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        dev = self.device.index if self.device.index is not None else -1
        with torch.cuda.stream(self.copy_stream):
            self.twins[i][:up.nbytes].copy_(self.ring[i][:up.nbytes], non_blocking=True)
            t["uploads"] += 1
            if up.tiles:
                twin = self.twins[i].data_ptr()
                _lib.check(_lib.load().dzn_ingest_many(
                    dev, C.c_void_p(twin), b.slot_bytes, C.c_void_p(self.ring[i].data_ptr()), C.c_void_p(twin), nd,
                    None if self.banks is None else C.c_void_p(self.banks.data_ptr()),
                    0 if self.banks is None else self.banks.numel(), C.c_void_p(self.pool.data_ptr()), b.max_sessions,
                    b.row_floats, C.c_void_p(self.copy_stream.cuda_stream)), None, "dzn_ingest_many")
                t["ingest_launches"] += 1
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.slot_free[i] = ev
        self.ingest_event = ev
        self.next_slot = (i + 1) % len(self.ring)

    def _upload_wave(self, up: ArrayUpload, t: dict) -> None:
        """one slot of an array wave: its image to the pinned slot, ONE H2D to the twin, ONE dzn_beamform_many, ONE
        dzn_ingest_many over the beamformed staging pool where a call resamples, the slot's event"""
        import torch
        b, a = self.book, self.arrays
        i = self.next_slot
        if self.slot_free[i] is not None:
            self.slot_free[i].synchronize()                                 # ring full: wait for the oldest copy and its kernels
        slot = self.ring_np[i]
        nd, nr = len(up.desc), len(up.rdesc)
        assert all(int(d["seen"]) == feed.seen for d, feed in zip(up.desc, up.keys))
        slot[:nd * ARRAY_DESC_BYTES] = up.desc.view(np.uint8)
        for off, data in up.chunks:
            slot[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        if nr:
            slot[up.roff:up.roff + nr * DESC_BYTES] = up.rdesc.view(np.uint8)
        dev = self.device.index if self.device.index is not None else -1
        vp, lib = C.c_void_p, _lib.load()
        with torch.cuda.stream(self.copy_stream):
            self.twins[i][:up.nbytes].copy_(self.ring[i][:up.nbytes], non_blocking=True)
            t["uploads"] += 1
            st, twin, host = vp(self.copy_stream.cuda_stream), self.twins[i].data_ptr(), self.ring[i].data_ptr()
            _lib.check(lib.dzn_beamform_many(
                dev, vp(twin), b.slot_bytes, vp(host), vp(twin), nd, vp(self.twiddles.data_ptr()), self.twiddles.numel(),
                vp(a["planar"].data_ptr()), b.planar_floats, vp(a["lag"].data_ptr()), vp(a["peak"].data_ptr()), b.temp_elems,
                vp(a["state"].data_ptr()), a["state"].numel(), vp(a["delay"].data_ptr()), a["delay"].numel(),
                vp(self.pool.data_ptr()), self.pool.numel(), vp(a["beam"].data_ptr()), a["beam"].numel(), st),
                None, "dzn_beamform_many")
            t["array_calls"] += nd
            t["array_launches"] += 1
            for feed, c in zip(up.keys, up.calls):
                feed.seen = c.b1
            if nr:
                _lib.check(lib.dzn_ingest_many(
                    dev, vp(a["beam"].data_ptr()), 4 * a["beam"].numel(), vp(host + up.roff), vp(twin + up.roff), nr,
                    vp(self.banks.data_ptr()), self.banks.numel(), vp(self.pool.data_ptr()), b.max_sessions, b.row_floats, st),
                    None, "dzn_ingest_many")
                t["ingest_launches"] += 1
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        for feed, c in zip(up.keys, up.calls):
            feed.n = c.m1
            feed.uploads += 1
        self.slot_free[i] = ev
        self.ingest_event = ev
        self.next_slot = (i + 1) % len(self.ring)

    def _forward(self, sessions, batches, total: int, want_emb: bool, t: dict, want_soft: bool = False):
        """the tick's forwards on the current stream, behind the ingest event -> (decisions u8 [total, L, S], embeddings f32
        [total, S, dim] or None, the one buffer that holds both, the soft scores f32 [total, L, S] — a device tensor of their
        own, not part of the buffer that goes to the host — or None)"""
        import torch
        r, eng = self.runner, self.runner.engine
        L, S = r.num_frames, eng.seg.max_speakers_per_chunk
        cur = torch.cuda.current_stream(self.device)
        self._wait_ingest()
        dim = eng.emb.embed_dim if want_emb else 0
        ne = total * S * dim * 4
        buf = torch.empty(ne + total * L * S, device=self.device, dtype=torch.uint8)
        seg_all = buf[ne:].view(total, L, S)
        emb_all = buf[:ne].view(torch.float32).view(total, S, dim) if want_emb else None
        soft_all = torch.empty((total, L, S), device=self.device, dtype=torch.float32) if want_soft else None
        offs = np.array([sessions[i].ingest.row * self.book.row_floats + (sessions[i].done + k) * self.book.step
                         for batch in batches for i, k in batch], dtype=np.int64)
        d_off = torch.from_numpy(offs).pin_memory().to(self.device, non_blocking=True)
        dev = self.device.index if self.device.index is not None else -1
        lib, b0 = _lib.load(), 0
        for batch in batches:
            B = len(batch)
            chunk = self.dense[:B]
            _lib.check(lib.dzn_gather_windows(dev, C.c_void_p(self.pool.data_ptr()), self.pool.numel(),
                                              C.c_void_p(offs[b0:].ctypes.data), C.c_void_p(d_off.data_ptr() + 8 * b0), B,
                                              r.window, C.c_void_p(chunk.data_ptr()), C.c_void_p(cur.cuda_stream)),
                       None, "dzn_gather_windows")
            if want_soft:
                _, ml, soft_all[b0:b0 + B] = eng.segment(chunk, want_logp=False, want_soft=True)
            else:
                _, ml = eng.segment(chunk, want_logp=False)
            filt, masks = eng.prepare_masks(ml, r.median_size, r.exclude_overlap,
                                            r.min_num_frames if r.exclude_overlap else -1, want_masks=want_emb)
            seg_all[b0:b0 + B] = filt
            if want_emb:
                emb_all[b0:b0 + B] = eng.embed(chunk, masks)
            b0 += B
            t["forwards"] += 1
        self._gathered = torch.cuda.Event()
        self._gathered.record(cur)
        return seg_all, emb_all, buf, soft_all

    def _release(self, sess) -> None:
        """a session has ended: its row is free; whoever takes it next zeroes [0, n + window) behind the last gather"""
        row = sess.ingest.row
        self.row_dirty[row] = (sess.ingest.n, self._gathered)
        del self.sessions[sess.name]
        self.book.release(sess.name, row)

    def close(self) -> None:
        """drop every session and the hub's buffers (sessions that have not ended get no final result)"""
        import torch
        if self.closed:
            return
        self.closed = True
        with torch.cuda.device(self.device):
            self.copy_stream.synchronize()
            torch.cuda.current_stream(self.device).synchronize()
        for s in list(self.sessions.values()):
            s.finished = True
        self.sessions.clear()
        self.pool = self.ring = self.ring_np = self.twins = self.dense = self.banks = self.arrays = self.twiddles = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
