"""The host half of a live hub's array feeds (diarizen_amd/hub.py), no device: how a tick's array calls are
grouped into waves and packed into staging slots (array_waves, pack_array_waves), the carry bookkeeping between a row's two
beamformed staging buffers (RowFeed.array_fields), what the book refuses, and that every call a slot can hold fits the
shared scratch and the row's tables."""
from __future__ import annotations

import numpy as np
import pytest

from diarizen_amd import _lib
from diarizen_amd.audio import ArrayFeedPlanner, Beamform, FeedFormat
from diarizen_amd.hub import (ALIGN, ARRAY_CALL_HOPS, ARRAY_DESC_BYTES, ARRAY_HISTORY, DESC_BYTES, STATE_INTS, HubBook, RowFeed,
                              array_waves, pack_array_waves)

TILE = BEAM_TILE = 1024                             # dzn_resample_tile / dzn_beamform_tile
SR, WINDOW, STEP = 16000, 128000, 12800
BF = Beamform(causal=True, hop=256, max_delay=8 / 16000)


def book(max_sessions=4, max_seconds=60.0, slot_bytes=1 << 16, array_channels=4, array_rate=48000):
    b = HubBook(max_sessions, max_seconds, SR, WINDOW, STEP, slot_bytes, TILE, array_channels, array_rate, BEAM_TILE)
    b.new_bank = lambda rate: 1000 * rate
    b.new_twiddle = lambda hop: 10 * hop             # a float offset per hop (the hub appends the table)
    return b


def fmt16(channels=4, enc="s16", bf=BF):
    return FeedFormat(16000, enc, channels=channels, channel=bf)


def pack(b):
    return pack_array_waves(b.take_array_queue(), b.slot_bytes, b.tile, b.beam_tile, b.planar_floats, b.temp_elems)


def frames(g, n, channels=4):
    return g.integers(-3000, 3000, size=(n, channels)).astype("<i2").tobytes()


def check_upload(up, b):
    """the table first, every call at a 16-byte boundary behind it, the resample table last, all inside the slot; the three
    prefixes and the scratch offsets consistent; no session twice"""
    d = up.desc
    assert d.dtype == _lib.beamform_desc_dtype() and d.dtype.itemsize == ARRAY_DESC_BYTES == 208
    assert up.nbytes <= b.slot_bytes and len(d) == len(up.keys) == len(up.calls)
    assert len(set(map(id, up.keys))) == len(up.keys) == len(set(d["state_offset"].tolist()))
    end = len(d) * ARRAY_DESC_BYTES
    dt = it = st = planar = temp = 0
    for i, (feed, c) in enumerate(zip(up.keys, up.calls)):
        r = d[i]
        assert r["src_offset"] == end and end % ALIGN == 0
        end += -(-len(c.data) // ALIGN) * ALIGN
        assert (r["decode_tile0"], r["gcc_item0"], r["sum_tile0"]) == (dt, it, st)
        assert (r["planar_offset"], r["lag_offset"]) == (planar, temp)
        C_ = feed.plan.fmt.channels
        assert (r["channels"], r["src_first"], r["src_frames"], r["T"]) == (C_, c.first, c.frames, c.total)
        assert (r["b0"], r["b1"], r["n0"], r["n1"], r["ch_stride"], r["blk_cap"]) == (c.b0, c.b1, c.n0, c.n1, c.frames, c.b1 - c.b0)
        assert (r["hop"], r["max_lag"], r["ref"]) == (feed.plan.hop, feed.plan.max_lag, feed.plan.beamform.reference)
        assert r["min_peak"] == np.float32(feed.plan.min_peak) and r["twiddle_offset"] == 10 * feed.plan.hop
        assert r["state_offset"] == feed.row * b.array_channels * STATE_INTS
        assert r["delay_offset"] == feed.row * b.array_channels * b.table_blocks and r["table_blocks"] == b.table_blocks
        assert r["s_first"] <= r["n0"] and len(c.data) == c.frames * feed.plan.fmt.frame_bytes
        dt += -(-c.frames // BEAM_TILE)
        it += (c.b1 - c.b0) * (C_ - 1)
        st += -(-(int(r["n1"]) - int(r["s_first"])) // BEAM_TILE)
        planar += C_ * c.frames
        temp += C_ * (c.b1 - c.b0)
    assert planar <= b.planar_floats and temp <= b.temp_elems
    assert up.roff == end and up.nbytes == end + len(up.rdesc) * DESC_BYTES
    assert [off for off, _ in up.chunks] == [int(o) for o, c in zip(d["src_offset"], up.calls) if len(c.data)]
    img = up.image()
    assert img[:len(d) * ARRAY_DESC_BYTES].tobytes() == d.tobytes() and img[up.roff:].tobytes() == up.rdesc.tobytes()
    tiles = 0
    for r in up.rdesc:
        assert r["tile0"] == tiles and r["src_format"] == 0 and r["channels"] == 1 and r["src_offset"] % 4 == 0
        tiles += -(-(int(r["m1"]) - int(r["m0"])) // TILE)


def test_one_wave_per_round_fields_prefixes_and_alignment():
    b = book()
    g = np.random.default_rng(3)
    a, c, u = b.admit(fmt16()), b.admit(fmt16(3)), b.admit(FeedFormat(8000, "ulaw", channels=2, channel=1))
    assert (a.array, c.array, u.array) == (True, True, False)
    seen_calls = 0
    for r in range(9):
        a.append(frames(g, 320 + r))
        c.append(frames(g, 517, 3) + (b"\x01" if r == 0 else b""))       # ends inside a frame once
        u.append(g.integers(0, 256, 1001, dtype=np.uint8).tobytes())
        assert [f for f, *_ in b.take_queue()] == [u] and all(f.array for f, _ in b.queue)
        ups = pack(b)
        assert len(ups) <= 1 and not b.queue
        for up in ups:
            check_upload(up, b)
            assert len(up.rdesc) == 0 and all(int(x) == 0 for x in up.desc["dst_space"])
            for d, feed, call in zip(up.desc, up.keys, up.calls):
                assert d["dst_offset"] == feed.row * b.row_floats + call.n0 and d["carry_offset"] == -1 and d["s_first"] == call.n0
                assert d["seen"] == call.b0
            seen_calls += len(up.calls)
    a.flush(), c.flush()
    (up,) = pack(b)
    check_upload(up, b)
    assert [int(x) for x in up.desc["n1"]] == [a.frames, c.frames] and seen_calls > 8
    assert a.staged == a.frames and c.staged == c.frames


def test_the_wave_rule():
    """queues with 1, 2 and 3 calls of one session interleaved with other sessions' calls"""
    for k in (1, 2, 3):
        for order in (["x"] * k + ["y", "z"], ["y"] + ["x"] * k + ["z", "y"], ["x", "y"] * k + ["z"], ["z", "x", "y", "x", "x"][:2 + k]):
            queue = [(key, i) for i, key in enumerate(order)]
            waves = array_waves(queue)
            flat = [e for w in waves for e in w]
            assert sorted(flat) == sorted(queue) and len(flat) == len(queue)             # every call exactly once
            for w in waves:
                assert len({key for key, _ in w}) == len(w)                                 # no wave holds two of a session
            for key in set(order):
                assert [i for k_, i in flat if k_ == key] == [i for k_, i in queue if k_ == key]      # a session's calls in order
            assert len(waves) == max(order.count(key) for key in set(order))
            for j, w in enumerate(waves):                                                   # wave j holds the j-th call of each
                assert all([i for k_, i in queue if k_ == key][j] == i for key, i in w)
    # through the packer: a session fed three blocks' worth before one tick takes three waves
    b = book()
    g = np.random.default_rng(4)
    x, y = b.admit(fmt16()), b.admit(fmt16())
    for _ in range(3):
        x.append(frames(g, 256))
    y.append(frames(g, 300))
    ups = pack(b)
    assert [[f.row for f in up.keys] for up in ups] == [[0, 1], [0], [0]]
    assert [int(up.desc["seen"][0]) for up in ups] == [0, 1, 2] and [int(up.desc["b1"][0]) for up in ups] == [1, 2, 3]
    for up in ups:
        check_upload(up, b)


def test_a_wave_that_exceeds_a_slot_is_split_in_order():
    b = book(max_sessions=6, slot_bytes=1 << 14)
    g = np.random.default_rng(5)
    feeds = [b.admit(fmt16()) for _ in range(6)]
    assert feeds[0].plan.slot_frames == min(b.array_max_call_bytes // 8 - 2 * 256 - 8, ARRAY_CALL_HOPS * 256) == 1024
    for f in feeds:
        f.append(frames(g, 600))                                                           # 4800 bytes each: three fit 16 KiB
    ups = pack(b)
    assert [[f.row for f in up.keys] for up in ups] == [[0, 1, 2], [3, 4, 5]]
    for up in ups:
        check_upload(up, b)
    # the scratch splits a wave as a slot does
    for f in feeds[:2]:
        f.append(frames(g, 300))
    calls = b.take_array_queue()
    ups = pack_array_waves(calls, b.slot_bytes, TILE, BEAM_TILE, 4 * 700, b.temp_elems)
    assert [len(up.keys) for up in ups] == [1, 1]
    with pytest.raises(ValueError, match="does not fit a staging slot"):
        pack_array_waves(calls, 1024, TILE, BEAM_TILE, b.planar_floats, b.temp_elems)


@pytest.mark.parametrize("slot_frames", [512, 3 * 512 + 5])
def test_carry_bookkeeping_over_random_chunkings_of_a_48k_feed(slot_frames):
    bf = Beamform(causal=True, hop=512, max_delay=24 / 48000)
    fmt = FeedFormat(48000, "s16", channels=4, channel=bf)
    g = np.random.default_rng(slot_frames)
    for trial in range(4):
        b = book(slot_bytes=1 << 16)
        feed = RowFeed(b, 1, ArrayFeedPlanner(fmt, SR, slot_frames))
        b.free.remove(1)
        total, holds, at = 14 * 512 + 3, {0: None, 1: None}, None          # holds[which] = (first, end) of what the buffer holds
        raw = frames(g, total)
        cuts = sorted(set(g.integers(0, len(raw), size=int(g.integers(2, 40))).tolist()) | {0, len(raw)})
        entries = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            feed.append(raw[lo:hi])
            entries += b.take_array_queue()
        feed.flush()
        entries += b.take_array_queue()
        assert [c.n0 for _, c, *_ in entries][1:] == [c.n1 for _, c, *_ in entries][:-1] and entries[-1][1].n1 == total
        made = 0
        for _, c, d, res, data in entries:
            assert d["seen"] == c.b0 and d["dst_space"] == 1
            if not (c.n1 > c.n0 or c.m1 > c.m0):
                assert d["s_first"] == c.n0 and res is None and d["carry_offset"] == -1
                continue
            which = (d["dst_offset"] - b.stage_offset(1, 0)) // b.stage_floats
            assert which in (0, 1) and d["dst_offset"] == b.stage_offset(1, which) and which != at      # the buffers alternate
            hist = c.n0 - d["s_first"]
            assert 0 <= hist < feed.plan.K <= ARRAY_HISTORY and hist + c.n1 - c.n0 <= b.stage_floats
            if hist:
                first, end = holds[which ^ 1]                                               # what the OTHER buffer holds
                assert first <= d["s_first"] and end == c.n0                                # never below it, and up to n0
                assert d["carry_offset"] == b.stage_offset(1, which ^ 1) + d["s_first"] - first
            else:
                assert d["carry_offset"] == -1
            holds[which], at = (d["s_first"], c.n1), which
            if c.m1 > c.m0:
                assert (res["src_offset"], res["src_first_index"], res["src_len"], res["total_len"]) == \
                    (4 * d["dst_offset"], d["s_first"], c.n1 - d["s_first"], c.n1)
                assert (res["m0"], res["m1"], res["dst_offset"]) == (c.m0, c.m1, 1 * b.row_floats + c.m0) and res["m0"] == made
                assert res["bank_offset"] == 1000 * 48000 and (res["o"], res["n"]) == (3, 1)
                made = c.m1
            else:
                assert res is None
        assert made == -(-total // 3) == feed.staged
        for up in pack_array_waves(entries, b.slot_bytes, TILE, BEAM_TILE, b.planar_floats, b.temp_elems):
            check_upload(up, b)
            assert len(up.keys) == 1


def test_refusals_take_nothing():
    b = book(max_sessions=3, array_channels=4, array_rate=16000)
    causal = Beamform(causal=True)
    for fmt, why in ((FeedFormat(16000, "s16", channels=5, channel=causal), "array_channels = 4"),
                     (FeedFormat(48000, "s16", channels=4, channel=causal), "array_rate = 16000"),
                     (FeedFormat(15999, "s16", channels=4, channel=causal), "does not fit in LDS"),
                     ("s16", "FeedFormat"), (FeedFormat(16000, "s16", channels=4), "channel choice")):
        with pytest.raises(ValueError, match=why):
            b.admit(fmt)
        assert len(b.free) == 3
    fmt = FeedFormat(16000, "s16", channels=4, channel=causal)
    fmt.channel = Beamform()                                             # (a FeedFormat refuses it itself: pin the hub's words)
    with pytest.raises(ValueError, match=r"FeedFormat: .* pass Beamform\(causal=True\)"):
        b.admit(fmt)
    # a call that cannot fit a staging slot: the default hop 4096 at 16 kHz, 2 hop + max_lag + 1 = 8353 frames of 8 bytes
    small = book(max_sessions=3, slot_bytes=1 << 16, array_rate=16000)
    assert causal.plan(16000, 4)[:2] == (4096, 160)
    with pytest.raises(ValueError, match=r"66824 bytes per call .* slot_bytes"):
        small.admit(FeedFormat(16000, "s16", channels=4, channel=causal))
    assert len(small.free) == 3 and len(b.free) == 3
    assert small.admit(fmt16()).row == 0 and b.admit(fmt16()).row == 0
    # the default book refuses as before, word for word
    plain = HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE)
    with pytest.raises(ValueError, match="is an array feed .channel=Beamform.: a hub's rows share one batched ingest launch, "
                                         "which does not beamform; open the session on its own"):
        plain.admit(fmt16())
    assert len(plain.free) == 2 and plain.array_memory() == dict(state=0, delay=0, staging=0, scratch=0)
    full = book(max_sessions=1)
    full.admit(fmt16())
    with pytest.raises(RuntimeError, match="max_sessions = 1"):
        full.admit(fmt16())


def test_open_hub_argument_validation():
    for bad in (1, 65, -1, 2.5, True, "4"):
        with pytest.raises(ValueError, match="array_channels"):
            HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE, bad)
    with pytest.raises(ValueError, match="array_rate needs array_channels"):
        HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE, 0, 48000)
    for bad in (0, -16000, 44100.0, True):
        with pytest.raises(ValueError, match="array_rate is a positive integer"):
            HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE, 4, bad)
    b = HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE, 2)
    assert (b.array_channels, b.array_rate) == (2, SR)                   # the default rate is the model's
    assert HubBook(2, 60.0, SR, WINDOW, STEP, 1 << 16, TILE, 64, 48000).array_rate == 48000
    import inspect
    from diarizen_amd.detection import VoiceActivityDetection
    from diarizen_amd.pipeline import DiariZenPipeline
    for fn in (DiariZenPipeline.open_hub, VoiceActivityDetection.open_hub):
        p = inspect.signature(fn).parameters
        assert p["array_channels"].default == 0 and p["array_rate"].default is None


@pytest.mark.parametrize("slot_bytes", [1 << 14, 1 << 16, 1 << 20])
def test_every_call_a_slot_can_hold_fits_the_scratch_and_the_tables(slot_bytes):
    """the worst calls per byte: one-byte samples (the most floats per byte), 64 channels on the smallest hop (the most lag /
    peak entries per byte) and calls without any frame (T = 0: a block and no byte)"""
    b = book(max_sessions=2, max_seconds=600.0, slot_bytes=slot_bytes, array_channels=64, array_rate=48000)
    assert b.planar_floats == b.temp_elems == slot_bytes
    assert b.table_blocks >= -(-int(600.0 * 48000) // 256) + 1           # the blocks of max_seconds at array_rate on hop 256
    mem = b.array_memory()
    assert mem == dict(state=4 * 2 * 64 * 5, delay=4 * 2 * 64 * b.table_blocks, staging=4 * 2 * 2 * (ARRAY_HISTORY + 4 * 4096),
                       scratch=12 * slot_bytes)
    for channels, enc, rate in ((2, "ulaw", 8000), (64, "ulaw", 8000), (64, "s16", 16000), (3, "u8", 48000)):
        fmt = FeedFormat(rate, enc, channels=channels, channel=Beamform(causal=True, hop=256, max_delay=0.001))
        max_lag = fmt.channel.plan(rate, channels)[1]
        if (2 * 256 + max_lag + 1) * fmt.frame_bytes > b.array_max_call_bytes:
            with pytest.raises(ValueError, match="slot_bytes"):
                b._admit_array(fmt)
            continue
        plan = b._admit_array(fmt)
        assert plan.max_upload_frames * fmt.frame_bytes <= b.array_max_call_bytes
        # as many of the largest calls as a slot holds, then as many empty ones: both sums stay inside the scratch
        per = ARRAY_DESC_BYTES + -(-plan.max_upload_frames * fmt.frame_bytes // ALIGN) * ALIGN
        k = slot_bytes // per
        assert k * channels * plan.max_upload_frames <= b.planar_floats
        assert k * channels * (plan.max_blocks + 2) <= b.temp_elems
        assert (slot_bytes // ARRAY_DESC_BYTES) * channels * 1 <= b.temp_elems
        assert plan.max_new <= 4 * 4096 and (plan.same_rate or plan.K + plan.max_new <= b.stage_floats)
