"""The host half of a live hub (diarizen_amd/hub.py), no device: how a tick's planned calls are packed into staging slots
(pack_tick), how its ready windows are spread over forwards (plan_batches), and what the book refuses (HubBook, RowFeed)."""
from __future__ import annotations

import numpy as np
import pytest

from diarizen_amd.audio import FeedFormat, resampled_length
from diarizen_amd.hub import ALIGN, DESC_BYTES, HubBook, pack_tick, plan_batches

TILE = 1024                                         # dzn_resample_tile (csrc/resample_tile.h)
SR, WINDOW, STEP = 16000, 128000, 12800


def book(max_sessions=4, max_seconds=60.0, slot_bytes=1 << 16):
    b = HubBook(max_sessions, max_seconds, SR, WINDOW, STEP, slot_bytes, TILE)
    b.new_bank = lambda rate: 1000 * rate            # a float offset per feed rate (the hub appends the bank)
    return b


def open_row(b, name, fmt):
    b.check_open(name)
    feed = b.admit(fmt)
    b.names[name] = feed.row
    return feed


def pack(b):
    return pack_tick([(feed, fields, data) for feed, _, fields, data in b.take_queue()], b.slot_bytes, b.tile)


def feed_rounds(b, seed, rounds, finish=True):
    """three sessions — an 8 kHz stereo mu-law call, a 48 kHz int16 microphone, float32 at the model's rate — fed interleaved in
    unequal chunks; -> (feeds by name, per round the uploads)"""
    g = np.random.default_rng(seed)
    feeds = {"ulaw": open_row(b, "ulaw", FeedFormat(8000, "ulaw", channels=2, channel=1)),
             "s16": open_row(b, "s16", FeedFormat(48000, "s16", channel=0)),
             "f32": open_row(b, "f32", None)}
    ticks = []
    for r in range(rounds):
        feeds["ulaw"].append(g.integers(0, 256, 5921, dtype=np.uint8).tobytes())
        feeds["s16"].append(g.integers(-2000, 2000, 7001 + 13 * r).astype("<i2"))
        if r % 2:
            feeds["f32"].append(g.standard_normal(5920).astype(np.float32))
        ticks.append(pack(b))
    if finish:
        for f in feeds.values():
            f.flush()
        ticks.append(pack(b))
    return feeds, ticks


def check_upload(up, slot_bytes):
    """the table first, every call at a 16-byte boundary behind it and inside the slot, the tile prefix consistent"""
    d = up.desc
    assert up.nbytes <= slot_bytes and len(d) == len(up.keys)
    end, tiles = len(d) * DESC_BYTES, 0
    assert [n for n in up.sizes if n] == [len(data) for _, data in up.chunks]
    for i in range(len(d)):
        assert d["src_offset"][i] % ALIGN == 0 and d["src_offset"][i] == end
        assert d["tile0"][i] == tiles
        end += -(-up.sizes[i] // ALIGN) * ALIGN
        tiles += -(-int(d["m1"][i] - d["m0"][i]) // TILE)
    assert end == up.nbytes and tiles == up.tiles
    img = up.image()
    assert img[:len(d) * DESC_BYTES].tobytes() == d.tobytes()
    for off, data in up.chunks:
        assert img[off:off + len(data)].tobytes() == data


@pytest.mark.parametrize("slot_bytes", [1 << 16, 1 << 14])
def test_ranges_tile_each_session_once_and_in_order(slot_bytes):
    b = book(slot_bytes=slot_bytes)
    feeds, ticks = feed_rounds(b, 3, 9)
    at = {f: 0 for f in feeds.values()}
    for ups in ticks:
        for up in ups:
            check_upload(up, slot_bytes)
            for i, feed in enumerate(up.keys):
                d = up.desc[i]
                assert d["m0"] == at[feed] and d["m1"] >= d["m0"]                 # in order, no gap, no overlap
                assert d["dst_offset"] == feed.row * b.row_floats + d["m0"]       # y[m0] inside the session's row
                assert (d["bank_offset"] < 0) == (feed.plan is None or feed.plan.same_rate)
                if feed.plan is not None and not feed.plan.same_rate:
                    assert d["bank_offset"] == 1000 * feed.plan.fmt.rate
                at[feed] = int(d["m1"])
    assert at[feeds["ulaw"]] == resampled_length(9 * 5921 // 2, 1, 2) == feeds["ulaw"].staged
    assert at[feeds["s16"]] == resampled_length(sum(7001 + 13 * r for r in range(9)), 3, 1)
    assert at[feeds["f32"]] == 4 * 5920
    if slot_bytes == 1 << 16:
        assert all(len(ups) == 1 for ups in ticks[:-1])                           # a tick that fits a slot is one upload


def test_a_tick_larger_than_a_slot_splits_without_reordering():
    slot = 1 << 12
    b = book(slot_bytes=slot)
    f = open_row(b, "a", FeedFormat(16000, "s16", channel=0))
    h = open_row(b, "b", None)
    x = np.arange(20000, dtype="<i2")
    f.append(x)                                                                   # 40 kB through 4 kB slots
    h.append(np.ones(3000, dtype=np.float32))
    f.append(x[:100])
    ups = pack(b)
    total = sum(DESC_BYTES + -(-len(c[1]) // ALIGN) * ALIGN for up in ups for c in up.chunks)
    assert len(ups) > 1 and len(ups) <= -(-total // (slot - slot // 2))           # as few as fit: every slot but the last over half full
    order = [(feed, int(up.desc["m0"][i]), int(up.desc["m1"][i])) for up in ups for i, feed in enumerate(up.keys)]
    for feed in (f, h):
        mine = [(m0, m1) for k, m0, m1 in order if k is feed]
        assert mine[0][0] == 0 and all(a[1] == b_[0] for a, b_ in zip(mine, mine[1:])) and mine[-1][1] == feed.staged
    for up in ups:
        check_upload(up, slot)
    # the stored bytes arrive unchanged and in order
    got = b"".join(up.image()[int(up.desc["src_offset"][i]):][:up.sizes[i]].tobytes() for up in ups
                   for i, k in enumerate(up.keys) if k is f)
    assert got == x.tobytes() + x[:100].tobytes()
    with pytest.raises(ValueError, match="does not fit a staging slot"):
        pack_tick([("k", dict(m0=0, m1=1), b"\0" * slot)], slot, TILE)


def test_empty_ranges_pack_to_zero_tiles():
    assert pack_tick([], 4096, TILE) == []
    ups = pack_tick([("a", dict(m0=5, m1=5, src_len=0), b""), ("b", dict(m0=0, m1=0, src_len=3), b"abc")], 4096, TILE)
    assert len(ups) == 1 and ups[0].tiles == 0 and list(ups[0].desc["tile0"]) == [0, 0]
    check_upload(ups[0], 4096)
    ups = pack_tick([("a", dict(m0=5, m1=5), b""), ("b", dict(m0=0, m1=1025), b"x" * 17), ("c", dict(m0=7, m1=7), b"")], 4096, TILE)
    assert ups[0].tiles == 2 and list(ups[0].desc["tile0"]) == [0, 0, 2]
    assert list(ups[0].desc["src_offset"]) == [3 * DESC_BYTES, 3 * DESC_BYTES, 3 * DESC_BYTES + 32]
    # a feed that makes nothing final plans no call at all
    b = book()
    f = open_row(b, "a", FeedFormat(8000, "ulaw", channel=0))
    assert f.append(b"\x7f" * 3) == 0 and pack(b) == []


@pytest.mark.parametrize("ready,batch_size", [([], 32), ([0, 0], 32), ([1], 32), ([3, 0, 2], 32), ([3, 0, 40], 32), ([29, 1, 11, 64], 32),
                                               ([5, 5, 5], 4), ([65], 64), ([1] * 64, 64), ([1] * 65, 64)])
def test_every_ready_window_is_scheduled_once_in_order_and_balanced(ready, batch_size):
    batches = plan_batches(ready, batch_size)
    total = sum(ready)
    assert len(batches) == -(-total // batch_size)                                # forwards = ceil(windows / batch_size); 0 -> 0
    flat = [w for batch in batches for w in batch]
    assert flat == [(i, k) for i, c in enumerate(ready) for k in range(c)]        # each once, sessions and windows in order
    sizes = [len(batch) for batch in batches]
    assert all(1 <= s <= batch_size for s in sizes)
    if sizes:
        bs = -(-total // len(sizes))                                              # run_views' balance: equal but a shorter last one
        assert sizes[:-1] == [bs] * (len(sizes) - 1) and 0 < sizes[-1] <= bs


def test_refusals_by_name_before_anything_is_taken(monkeypatch):
    b = book(max_sessions=2, max_seconds=10.0)
    with pytest.raises(ValueError, match="FeedFormat"):
        open_row(b, "x", "ulaw")
    with pytest.raises(ValueError, match="channel choice"):
        open_row(b, "x", FeedFormat(8000, "ulaw", channels=2))                    # (the session settles the channel first)
    with pytest.raises(ValueError, match="does not fit in LDS"):
        open_row(b, "x", FeedFormat(15999, "s16", channel=0))
    assert b.free == [0, 1] and not b.names                                       # nothing was taken
    a = open_row(b, "a", FeedFormat(8000, "s16", channel=0))
    with pytest.raises(ValueError, match="already open"):
        open_row(b, "a", None)
    with pytest.raises(ValueError, match="needs a name"):
        open_row(b, None, None)
    c = open_row(b, "c", None)
    assert (a.row, c.row) == (0, 1)
    with pytest.raises(RuntimeError, match="max_sessions = 2"):
        open_row(b, "d", None)
    # a stream longer than max_seconds, as a solo session refuses it
    a.append(np.zeros(8000 * 9, dtype="<i2"))
    with pytest.raises(MemoryError, match="max_seconds = 10 s"):
        a.append(np.zeros(8000 * 2, dtype="<i2"))
    c.append(np.zeros(16000 * 9, dtype=np.float32))
    with pytest.raises(MemoryError, match="max_seconds = 10 s"):
        c.append(np.zeros(16001, dtype=np.float32))
    c.append(np.zeros(16000, dtype=np.float32))
    # feed after the end of the stream
    c.flush()
    with pytest.raises(RuntimeError, match="already finished"):
        c.append(np.zeros(1, dtype=np.float32))
    a.flush()
    with pytest.raises(RuntimeError, match="already finished"):
        a.append(b"\0\0")
    # a released row goes to the next session
    b.release("a", a.row)
    assert open_row(b, "a", None).row == 0
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_sessions"):
            HubBook(bad, 10.0, SR, WINDOW, STEP, 1 << 16, TILE)
    with pytest.raises(ValueError, match="max_seconds"):
        HubBook(1, 0.0, SR, WINDOW, STEP, 1 << 16, TILE)


def test_a_hub_runs_on_one_rank(monkeypatch):
    """torch.distributed with more than one rank is refused before the hub looks at the pipeline (or allocates)"""
    from diarizen_amd import dist as dz_dist
    from diarizen_amd.hub import LiveHub
    monkeypatch.setattr(dz_dist, "world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="LiveHub runs on one device"):
        LiveHub(None, None)


def test_descriptor_record_is_the_c_struct():
    import ctypes as C
    from diarizen_amd import _lib
    dt = _lib.ingest_desc_dtype()
    assert dt.itemsize == DESC_BYTES == C.sizeof(_lib.DznIngestDesc)
    for name, _ in _lib.DznIngestDesc._fields_:
        assert dt.fields[name][1] == getattr(_lib.DznIngestDesc, name).offset
