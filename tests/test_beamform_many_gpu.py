"""dzn_beamform_many on the MI355X (csrc/beamform_many.hip): one table over several array rows, driven wave by
wave as a hub's tick drives it (hub.RowFeed, hub.pack_array_waves), beside dzn_beamform_feed on the SAME planned calls (the
solo ingest, streaming.WaveIngest._run_array, with buffers of its own).  Every comparison is exact: lag and peak per call, the
final tracker state, the whole delay table, the output rows; the sentinels around every buffer stay untouched.  The signals are
P, Q, R of testkit/beamform_live_ref.py: hop 256 / 512, 4 channels, T of 3.6 k / 7.2 k — the smallest shapes with several
blocks, a ragged tail, mixed hops in one launch and more than one tile per call."""
from __future__ import annotations

import audioop
import ctypes as C

import numpy as np
import pytest
import torch

from testkit import beamform_live_ref as LR

pytestmark = pytest.mark.gpu

PACKET = 5921
G = 64                                               # guard elements on either side of every buffer
F_SENT, I_SENT, B_SENT, POOL_FILL = -7.0, 99, 0xA5, -3.0
SR, WINDOW, STEP = 16000, 1600, 160


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


class Guarded:
    """a device buffer of n elements between two guards of G sentinels"""

    def __init__(self, n, dtype, sentinel, fill, gpu):
        self.n, self.sentinel = n, sentinel
        self.whole = torch.full((n + 2 * G,), sentinel, device=gpu, dtype=dtype)
        self.t = self.whole[G:G + n]
        self.t.fill_(fill)

    def intact(self) -> bool:
        return bool((self.whole[:G] == self.sentinel).all() and (self.whole[G + self.n:] == self.sentinel).all())


class Rig:
    """the device half of a hub's array waves without the hub: the book and the packer are the product's, the buffers are
    guarded and the launches are made here"""

    def __init__(self, lib, gpu, rows=3, channels=4, rate=48000, slot_bytes=1 << 16):
        from diarizen_amd import audio
        from diarizen_amd.hub import STATE_INTS, HubBook
        self.lib, self.gpu = lib, gpu
        self.book = b = HubBook(rows, 1.0, SR, WINDOW, STEP, slot_bytes, audio.resample_tile(), channels, rate, audio.beamform_tile())
        b.new_twiddle, b.new_bank = self._new_twiddle, self._new_bank
        self.tw_host, self.bank_host = np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32)
        self.twiddles = self.banks = None
        f32, i32 = torch.float32, torch.int32
        self.stage = Guarded(slot_bytes, torch.uint8, B_SENT, 0, gpu)
        self.planar = Guarded(b.planar_floats, f32, F_SENT, F_SENT, gpu)
        self.lag = Guarded(b.temp_elems, i32, I_SENT, I_SENT, gpu)
        self.peak = Guarded(b.temp_elems, f32, F_SENT, F_SENT, gpu)
        self.state = Guarded(rows * channels * STATE_INTS, i32, I_SENT, 0, gpu)
        self.delay = Guarded(rows * channels * b.table_blocks, i32, I_SENT, 0, gpu)
        self.pool = Guarded(rows * b.row_floats, f32, F_SENT, POOL_FILL, gpu)
        self.beam = Guarded(rows * 2 * b.stage_floats, f32, F_SENT, F_SENT, gpu)
        self.launches = 0

    def buffers(self):
        return [self.stage, self.planar, self.lag, self.peak, self.state, self.delay, self.pool, self.beam]

    def _new_twiddle(self, hop):
        from diarizen_amd.audio import beamform_twiddle
        off = len(self.tw_host)
        self.tw_host = np.concatenate([self.tw_host, beamform_twiddle(hop).reshape(-1)])
        self.twiddles = Guarded(len(self.tw_host), torch.float32, F_SENT, 0, self.gpu)
        self.twiddles.t.copy_(torch.from_numpy(self.tw_host))
        return off

    def _new_bank(self, rate):
        from diarizen_amd.audio import _device_bank
        off = len(self.bank_host)
        self.bank_host = np.concatenate([self.bank_host, _device_bank(rate, SR, self.gpu)[0].reshape(-1).cpu().numpy()])
        self.banks = torch.from_numpy(self.bank_host).to(self.gpu)
        return off

    def open(self, fmt, slot_frames=None):
        """a row for `fmt`: the book's own planner, or one with `slot_frames` new frames per call"""
        from diarizen_amd.audio import ArrayFeedPlanner
        from diarizen_amd.hub import RowFeed
        if slot_frames is None:
            return self.book.admit(fmt)
        return RowFeed(self.book, self.book.free.pop(0), ArrayFeedPlanner(fmt, SR, slot_frames))

    def many(self, desc, host=None):
        """dzn_beamform_many over the table `desc` (the stage holds its image already) -> (rc, message)"""
        b, gpu = self.book, self.gpu
        host = np.ascontiguousarray(desc) if host is None else host
        tw = self.twiddles
        rc = self.lib.dzn_beamform_many(
            gpu.index, _ptr(self.stage.t), b.slot_bytes, C.c_void_p(host.ctypes.data), _ptr(self.stage.t), len(desc),
            _ptr(tw.t), tw.n, _ptr(self.planar.t), self.planar.n, _ptr(self.lag.t), _ptr(self.peak.t), self.lag.n,
            _ptr(self.state.t), self.state.n, _ptr(self.delay.t), self.delay.n, _ptr(self.pool.t), self.pool.n,
            _ptr(self.beam.t), self.beam.n, _stream(gpu))
        return rc, self.lib.dzn_last_error(None).decode()

    def put(self, up):
        img = up.image()
        self.stage.t[:len(img)].copy_(torch.from_numpy(img))
        return img

    def run(self, up):
        """one upload of a wave: the image, dzn_beamform_many, dzn_ingest_many over the staging pool where a call resamples"""
        b, gpu = self.book, self.gpu
        assert all(int(d["seen"]) == feed.seen for d, feed in zip(up.desc, up.keys))
        self.put(up)
        rc, msg = self.many(up.desc)
        assert rc == 0, msg
        self.launches += 1
        for feed, c in zip(up.keys, up.calls):
            feed.seen = c.b1
        if len(up.rdesc):
            rdesc = np.ascontiguousarray(up.rdesc)
            rc = self.lib.dzn_ingest_many(gpu.index, _ptr(self.beam.t), 4 * self.beam.n, C.c_void_p(rdesc.ctypes.data),
                                          _ptr(self.stage.t, up.roff), len(rdesc), _ptr(self.banks), self.banks.numel(),
                                          _ptr(self.pool.t), b.max_sessions, b.row_floats, _stream(gpu))
            assert rc == 0, self.lib.dzn_last_error(None).decode()
        torch.cuda.synchronize(gpu)
        for feed, c in zip(up.keys, up.calls):
            feed.n = c.m1

    def waves(self):
        from diarizen_amd.hub import pack_array_waves
        b = self.book
        return pack_array_waves(b.take_array_queue(), b.slot_bytes, b.tile, b.beam_tile, b.planar_floats, b.temp_elems)

    def row_state(self, feed):
        from diarizen_amd.hub import STATE_INTS
        n = self.book.array_channels * STATE_INTS
        return self.state.t[feed.row * n:(feed.row + 1) * n].view(self.book.array_channels, STATE_INTS)

    def row_delay(self, feed):
        n = self.book.array_channels * self.book.table_blocks
        return self.delay.t[feed.row * n:(feed.row + 1) * n].view(self.book.array_channels, self.book.table_blocks)

    def row_wave(self, feed):
        return self.pool.t[feed.row * self.book.row_floats:(feed.row + 1) * self.book.row_floats]


def _solo(gpu, feed):
    """the solo ingest that runs the SAME planned calls through dzn_beamform_feed (and dzn_resample), buffers of its own"""
    from diarizen_amd.streaming import WaveIngest
    p = feed.plan
    ing = WaveIngest(gpu, SR, WINDOW, STEP, max_seconds=1.0, slot_seconds=1.0, slots=3, feed_format=p.fmt, slot_frames=p.slot_frames)
    ing.plan = p                                      # one planner: the calls the rig packs are the calls this ingest runs
    return ing


def _drive(rig, gpu, rows, check_lag=True):
    """rows: [(feed, chunks)] fed round robin, one chunk per row and round, flushed when a row's chunks are out, the waves of
    every round run on the rig and, call by call, on each row's solo ingest; lag / peak are compared per call.
    -> the solo ingests"""
    solos = [_solo(gpu, feed) for feed, _ in rows]
    by_feed = {id(feed): s for (feed, _), s in zip(rows, solos)}
    todo = [list(chunks) for _, chunks in rows]
    live = set(range(len(rows)))
    while live:
        for i in sorted(live):
            feed = rows[i][0]
            if todo[i]:
                feed.append(todo[i].pop(0))
            else:
                feed.flush()
                live.discard(i)
        for up in rig.waves():
            rig.run(up)
            for d, feed, c in zip(up.desc, up.keys, up.calls):
                s = by_feed[id(feed)]
                s._run_array([c])
                s.copy_stream.synchronize()
                n = int(d["channels"]) * (c.b1 - c.b0)
                if check_lag and n:
                    at = int(d["lag_offset"])
                    assert torch.equal(rig.lag.t[at:at + n], s._lag.reshape(-1)[:n]), (feed.row, c.b0, c.b1)
                    assert torch.equal(rig.peak.t[at:at + n], s._peak.reshape(-1)[:n]), (feed.row, c.b0, c.b1)
    return solos


def _compare(rig, feed, solo):
    """final state, the whole delay table and the output row against the solo ingest"""
    Cn, nb = feed.plan.fmt.channels, feed.plan.blocks
    assert feed.seen == nb == solo._seen.value and feed.n == solo.n
    st, dl, wave = rig.row_state(feed), rig.row_delay(feed), rig.row_wave(feed)
    assert torch.equal(st[:Cn], solo._state) and not st[Cn:].any()
    assert torch.equal(dl[:Cn, :nb], solo._delay[:, :nb]) and not dl[:Cn, nb:].any() and not dl[Cn:].any()
    assert not solo._delay[:, nb:].any()
    assert torch.equal(wave[:feed.n], solo.dev_wave[:feed.n]), feed.row
    assert bool((wave[feed.n:] == POOL_FILL).all())                      # nothing is written behind the recording
    assert all(b.intact() for b in rig.buffers()) and rig.twiddles.intact()


def _bf(c, rate=16000, **kw):
    from diarizen_amd.audio import Beamform
    return Beamform(causal=True, hop=c["hop"], max_delay=c["max_lag"] / rate, **kw)


def _chunkings(raw: bytes, hop: int, frame_bytes: int):
    """(chunks, slot_frames): one chunk, 5921-byte packets (which end inside a frame), and chunks of 2 hop - 1 frames into
    slots of hop frames, so that every chunk is split"""
    step = (2 * hop - 1) * frame_bytes
    return [([raw], None), ([raw[i:i + PACKET] for i in range(0, len(raw), PACKET)], None),
            ([raw[i:i + step] for i in range(0, len(raw), step)], hop)]


@pytest.mark.parametrize("chunking", [0, 1, 2])
def test_one_table_over_p_q_r_equals_the_single_calls(built_lib, gpu, chunking):
    from diarizen_amd.audio import FeedFormat
    rig = Rig(built_lib, gpu)
    rows = []
    for name in ("P", "Q", "R"):
        c = LR.signal(name)
        fmt = FeedFormat(16000, "s16", channels=4, channel=_bf(c))
        chunks, slot_frames = _chunkings(LR.frames_of(c["x"]).tobytes(), c["hop"], fmt.frame_bytes)[chunking]
        rows.append((rig.open(fmt, slot_frames), chunks))
    solos = _drive(rig, gpu, rows)
    hops = {f.plan.hop for f, _ in rows}
    assert hops == {256, 512} and len(rig.book.twiddle_offsets) == 2    # mixed hops in one launch, a table per hop
    for (feed, _), solo, name in zip(rows, solos, "PQR"):
        _compare(rig, feed, solo)
        assert feed.n == LR.signal(name)["T"]
        assert np.array_equal(rig.row_delay(feed)[:4, :feed.seen].cpu().numpy(), LR.reference_delays(name))
    assert rig.launches < sum(s.uploads for s in solos)                 # several calls shared a launch set


def test_two_and_three_channels_with_the_last_as_reference(built_lib, gpu):
    """C = 2, and C = 3 with ref = 2: the reference row is written by the workgroup of the lowest OTHER channel, and the
    work items skip the reference"""
    from diarizen_amd.audio import FeedFormat
    rig = Rig(built_lib, gpu)
    c = LR.signal("P")
    x = c["x"]
    rows = []
    for pick, ref in (((0, 3), 0), ((1, 0), 1), ((1, 3, 0), 2)):
        fmt = FeedFormat(16000, "s16", channels=len(pick), channel=_bf(c, reference=ref))
        raw = LR.frames_of(x[list(pick)]).tobytes()
        rows.append((rig.open(fmt), [raw[i:i + PACKET] for i in range(0, len(raw), PACKET)]))
    solos = _drive(rig, gpu, rows)
    for (feed, _), solo in zip(rows, solos):
        _compare(rig, feed, solo)
        d = rig.row_delay(feed)[:feed.plan.fmt.channels, :feed.seen]
        assert not d[feed.plan.beamform.reference].any() and d.any()    # the reference row is 0, the others found delays


def test_formats_in_one_table(built_lib, gpu):
    """s16, mu-law and interleaved float32 rows in one table, with 257 / 256 / 1 new frames per planned call"""
    from diarizen_amd.audio import FeedFormat
    rig = Rig(built_lib, gpu)
    c = LR.signal("P")
    pcm = LR.frames_of(c["x"])
    raws = {"s16": pcm.tobytes(), "ulaw": audioop.lin2ulaw(pcm.tobytes(), 2),
            "f32": np.ascontiguousarray(c["x"].T, dtype=np.float32).tobytes()}
    rows = []
    for (enc, raw), slot_frames in zip(raws.items(), (257, 256, 1)):
        fmt = FeedFormat(16000, enc, channels=4, channel=_bf(c))
        assert fmt.src_format == {"s16": 1, "ulaw": 6, "f32": 5}[enc]
        step = 997 * fmt.frame_bytes + 1                                 # chunks end inside a frame
        rows.append((rig.open(fmt, slot_frames), [raw[i:i + step] for i in range(0, len(raw), step)]))
    solos = _drive(rig, gpu, rows)
    for (feed, _), solo in zip(rows, solos):
        _compare(rig, feed, solo)
        assert feed.n == c["T"] and rig.row_wave(feed)[:feed.n].any()
    assert torch.equal(rig.row_wave(rows[0][0])[:c["T"]], rig.row_wave(rows[2][0])[:c["T"]])      # int16 values either way


def test_degenerate_calls(built_lib, gpu):
    """T = 100 (finish only), T = 0, all-silent channels, and a descriptor with b1 == b0 beside them"""
    from diarizen_amd.audio import FeedFormat
    rig = Rig(built_lib, gpu, rows=4)
    c = LR.signal("P")
    fmt = FeedFormat(16000, "s16", channels=4, channel=_bf(c))
    silent = np.array(c["x"][:, :5 * 256 + 9])
    silent[1:] = 0
    raws = [LR.frames_of(c["x"][:, :100]).tobytes(), b"", LR.frames_of(silent).tobytes()]
    rows = [(rig.open(fmt), [raw[i:i + PACKET] for i in range(0, len(raw), PACKET)]) for raw in raws]
    idle = rig.open(fmt)
    solos = _drive(rig, gpu, rows)
    for (feed, _), solo, T in zip(rows, solos, (100, 0, 5 * 256 + 9)):
        _compare(rig, feed, solo)
        assert feed.n == T and not rig.row_delay(feed).any()
    assert rig.row_wave(rows[0][0])[:100].any() and rig.row_wave(rows[2][0])[:5 * 256 + 9].any()
    # a descriptor that completes no block and makes no sample, first in a table beside a real call of another row
    from diarizen_amd import _lib
    assert not rig.book.free
    idle.append(LR.frames_of(c["x"][:, :300]).tobytes())
    (up,) = rig.waves()
    feed0 = rows[0][0]
    desc = np.zeros(2, dtype=_lib.beamform_desc_dtype())
    desc[1] = up.desc[0]
    desc[0] = up.desc[0]
    for k, v in dict(src_frames=0, ch_stride=0, T=100, src_first=0, b0=feed0.seen, b1=feed0.seen, seen=feed0.seen, blk_cap=0, n0=100,
                     n1=100, s_first=100, state_offset=feed0.row * rig.book.array_channels * 5,
                     delay_offset=feed0.row * rig.book.array_channels * rig.book.table_blocks,
                     dst_offset=feed0.row * rig.book.row_floats + 100, planar_offset=0, lag_offset=0).items():
        desc[0][k] = v
    # the image the device reads: the table of TWO descriptors, then the real call's bytes behind it
    (off, data), = up.chunks
    desc[1]["src_offset"] = desc[0]["src_offset"] = 2 * desc.dtype.itemsize
    img = np.concatenate([desc.view(np.uint8), np.frombuffer(data, dtype=np.uint8)])
    rig.stage.t[:len(img)].copy_(torch.from_numpy(img))
    before = [b.whole.clone() for b in (rig.state, rig.delay, rig.pool)]
    rc, msg = rig.many(desc)
    torch.cuda.synchronize(gpu)
    assert rc == 0, msg
    n = rig.book.array_channels * 5
    after_state = rig.state.whole.clone()
    assert not torch.equal(after_state, before[0])                      # the real call ran ...
    after_state[G + idle.row * n:G + (idle.row + 1) * n] = before[0][G + idle.row * n:G + (idle.row + 1) * n]
    assert torch.equal(after_state, before[0])                          # ... and nothing of the idle descriptor's row moved
    assert torch.equal(rig.pool.whole, before[2]) and all(b.intact() for b in rig.buffers())
    assert rig.many(desc[:0])[0] == 0                                   # an empty table


@pytest.mark.parametrize("chunking", [0, 1, 2])
def test_r_at_48k_into_a_16k_pool_equals_the_solo_ingest(built_lib, gpu, chunking):
    """the carry path and the dzn_ingest_many behind it: beamformed at 48 kHz into the two staging buffers, resampled from them"""
    from diarizen_amd.audio import FeedFormat, resampled_length
    rig = Rig(built_lib, gpu)
    c = LR.signal("R")
    fmt = FeedFormat(48000, "s16", channels=4, channel=_bf(c, 48000))
    chunks, slot_frames = _chunkings(LR.frames_of(c["x"]).tobytes(), c["hop"], fmt.frame_bytes)[chunking]
    p = LR.signal("P")                                                  # a 16 kHz row beside it: both destinations in one table
    raw = LR.frames_of(p["x"]).tobytes()
    rows = [(rig.open(fmt, slot_frames), chunks),
            (rig.open(FeedFormat(16000, "s16", channels=4, channel=_bf(p))), [raw[i:i + PACKET] for i in range(0, len(raw), PACKET)])]
    solos = _drive(rig, gpu, rows)
    for (feed, _), solo in zip(rows, solos):
        _compare(rig, feed, solo)
    feed = rows[0][0]
    assert feed.n == resampled_length(c["T"], 3, 1) and feed.plan.frames == c["T"] and rig.row_wave(feed)[:feed.n].any()
    assert np.array_equal(rig.row_delay(feed)[:4, :feed.seen].cpu().numpy(), LR.reference_delays("R"))


def test_refusals_leave_every_buffer_untouched_and_name_the_descriptor(built_lib, gpu):
    from diarizen_amd.audio import FeedFormat
    rig = Rig(built_lib, gpu)
    r = LR.signal("R")
    fmt48 = FeedFormat(48000, "s16", channels=4, channel=_bf(r, 48000))
    p = LR.signal("P")
    rows = [rig.open(FeedFormat(16000, "s16", channels=4, channel=_bf(p))), rig.open(fmt48)]
    rows[0].append(LR.frames_of(p["x"][:, :3 * 256 + 5]).tobytes())
    rows[1].append(LR.frames_of(r["x"][:, :1536 + 7]).tobytes())
    rig.run(rig.waves()[0])                                             # three blocks each: the second calls carry history
    rows[0].append(LR.frames_of(p["x"][:, 3 * 256 + 5:5 * 256]).tobytes())
    rows[1].append(LR.frames_of(r["x"][:, 1536 + 7:2600]).tobytes())
    (up,) = rig.waves()
    assert len(up.desc) == 2 and up.desc["carry_offset"][1] >= 0 and up.desc["dst_space"].tolist() == [0, 1]
    rig.put(up)
    torch.cuda.synchronize(gpu)
    before = [b.whole.clone() for b in rig.buffers()]
    b = rig.book
    good = up.desc
    cases = [
        (1, dict(state_offset=int(good["state_offset"][0])), "two calls of one session"),
        (0, dict(seen=int(good["seen"][0]) + 1), "out of sequence"),
        (1, dict(seen=0), "out of sequence"),
        (0, dict(planar_offset=b.planar_floats - 1), "leaves the"),
        (1, dict(planar_offset=int(good["planar_offset"][0]) + 1), "scratch overlaps that of descriptor 0"),
        (1, dict(lag_offset=b.temp_elems), "lag / peak rows"),
        (1, dict(lag_offset=int(good["lag_offset"][0])), "scratch overlaps"),
        (0, dict(state_offset=rig.state.n - 19), "ints of d_state"),
        (1, dict(delay_offset=rig.delay.n - 4 * b.table_blocks + 1), "ints of d_delay"),
        (0, dict(dst_offset=rig.pool.n - 1), "floats of d_pool"),
        (1, dict(dst_offset=rig.beam.n - 1), "floats of d_beam"),
        (1, dict(dst_offset=int(good["carry_offset"][1])), "lie in the range the call writes"),
        (1, dict(carry_offset=rig.beam.n), "carried samples"),
        (1, dict(s_first=int(good["n0"][1]) + 1), "s_first"),
        (1, dict(src_offset=b.slot_bytes - 8), "bytes of d_stage"),
        (0, dict(src_offset=int(good["src_offset"][0]) + 1), "not aligned"),
        (0, dict(twiddle_offset=rig.twiddles.n), "floats of d_twiddles"),
        (1, dict(decode_tile0=int(good["decode_tile0"][1]) + 1), "are not the tile prefixes"),
        (1, dict(gcc_item0=0), "are not the tile prefixes"),
        (1, dict(sum_tile0=int(good["sum_tile0"][1]) - 1), "are not the tile prefixes"),
        (0, dict(channels=1), "1 channel"), (0, dict(channels=65), "65 channel"), (1, dict(ref=4), "reference channel 4"),
        (0, dict(hop=300), "hop 300"), (1, dict(max_lag=0), "max_lag 0"), (0, dict(max_lag=129), "max_lag 129"),
        (0, dict(src_format=8), "src_format 8"), (0, dict(src_format=0), "float32 mono"),
        (1, dict(blk_cap=0), "do not fit"), (0, dict(table_blocks=4), "do not fit"),
        (0, dict(n1=int(good["T"][0]) + 1), "are not inside the recording"),
        (0, dict(n1=int(good["n1"][0]) + 256), "are tracked after this call"),
        (1, dict(src_first=int(good["src_first"][1]) + 1, src_frames=int(good["src_frames"][1]) - 1), "does not cover"),
        (0, dict(ch_stride=int(good["src_frames"][0]) - 1), "ch_stride"),
        (1, dict(dst_space=2), "dst_space"), (0, dict(reserved0=1), "reserved"),
    ]
    for at, change, why in cases:
        desc = good.copy()
        for k, v in change.items():
            desc[k][at] = v
        rc, msg = rig.many(desc)
        assert rc == -1 and msg.startswith(f"dzn_beamform_many: descriptor {at}: ") and why in msg, (at, change, rc, msg)
    b_ = rig.book
    rc = rig.lib.dzn_beamform_many(gpu.index, _ptr(rig.stage.t), b_.slot_bytes, None, _ptr(rig.stage.t), 2, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, _stream(gpu))
    assert rc == -1 and "null pointer" in rig.lib.dzn_last_error(None).decode()
    torch.cuda.synchronize(gpu)
    for buf, was in zip(rig.buffers(), before):                         # a refused call launches nothing
        assert torch.equal(buf.whole, was)
    rig.run(up)                                                         # and the table itself is sound
    assert rows[0].seen == 5 and rows[1].seen == 5 and all(x.intact() for x in rig.buffers())
