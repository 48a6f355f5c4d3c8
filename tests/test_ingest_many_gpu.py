"""dzn_ingest_many (csrc/ingest.hip, ops.ingest_many) on the MI355X: ONE launch over a shuffled table of descriptors — every
stored format, one / two / three channels with an index and with the downmix, 8 / 11.025 / 32 / 44.1 / 48 kHz -> 16 kHz and
16 kHz itself (decode only), ranges on and off the 1024-sample tile, the first and the last range of a recording and an empty
one.  Every descriptor's output must be torch.equal to the single dzn_resample / dzn_decode call with the same arguments
(tests/test_resample_gpu.py and tests/test_decode_gpu.py pin those to the host form and to float64), and no other float of the
pool may change.  Then the refusals: the whole call fails, names the descriptor, launches nothing."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from testkit.feeds import stored_forms

pytestmark = pytest.mark.gpu

MODEL_RATE = 16000
# (feed rate, stored format, channels, channel); 32000 has an even o: the padded LDS image.  Recordings of <= 5000 frames.
CONFIGS = [(8000, "ulaw", 2, 1), (8000, "alaw", 2, "downmix"), (11025, "s16", 1, 0), (32000, "s24", 3, 2),
           (44100, "s32", 2, "downmix"), (48000, "f32", 1, 0), (48000, "f32", 3, "downmix"), (32000, "u8", 1, 0),
           (11025, "u8", 3, "downmix"), (44100, "alaw", 1, 0), (8000, "s16", 3, 0), (48000, "s24", 2, 0),
           (16000, "s16", 2, 1), (16000, "ulaw", 3, "downmix"), (16000, "f32", 1, 0), (16000, "s32", 1, 0)]
FRAMES = {8000: 2500, 11025: 3400, 32000: 5000, 44100: 5000, 48000: 5000, 16000: 4100}
SENTINEL = -77.25
ROW, ROWS = 16384, 8


class Table:
    """the descriptors, the staging bytes, the banks and, per descriptor, what the single call gives"""


@pytest.fixture(scope="module")
def table(built_lib, gpu):
    from diarizen_amd import _lib
    from diarizen_amd.audio import (SRC_FORMATS, _device_bank, decode_device, resample_device, resample_input_span,
                                    resample_ratio, resample_tile, resampled_length)
    assert resample_tile() == 1024
    g = np.random.default_rng(2024)
    banks, bank_at, nbank = [], {}, 0
    for rate in sorted({c[0] for c in CONFIGS} - {MODEL_RATE}):
        bank = _device_bank(rate, MODEL_RATE, gpu)[0].reshape(-1)
        banks.append(bank)
        bank_at[rate], nbank = nbank, nbank + bank.numel()
    entries = []                                     # (fields, stored bytes, reference tensor)
    for ci, (rate, name, C, ch) in enumerate(CONFIGS):
        T = FRAMES[rate]
        stored = stored_forms(T, C, seed=300 + ci)[name][0]
        code = 5 if name == "f32" and C > 1 else SRC_FORMATS[name]
        flat = np.ascontiguousarray(stored).reshape(T, -1)               # one row per frame
        chan = -1 if ch == "downmix" else ch
        if rate == MODEL_RATE:
            o, n, width, out_len = 1, 1, 0, T
        else:
            o, n, width = resample_ratio(rate, MODEL_RATE)
            out_len = resampled_length(T, o, n)
        # on and off the tile, the first range (left zero fill), the last one (right zero fill, ending at ceil(n T / o)), empty;
        # 5000 frames at 44.1 / 48 kHz are fewer than 2048 samples: there the last range is the one that crosses tiles
        ranges = [(0, 1), (1023, 1025), (1024, 2048), (1000, 2025), (0, 700), (out_len - 1500, out_len), (5, 5)]
        ranges = [r for r in ranges if r[1] <= out_len]
        assert out_len > 1600 and len(ranges) >= 5 and (len(ranges) == 7 or rate > 32000)
        for ri, (m0, m1) in enumerate(ranges):
            if rate == MODEL_RATE:
                lo, hi = m0, m1
                ref = decode_device(flat[lo:hi].reshape(-1), device=gpu, channels=C, channel=ch, src_format=name)
            else:
                lo, hi = resample_input_span(m0, m1, o, n, width)
                lo, hi = max(lo, 0), max(min(hi, T), 0)
                if ri % 2 and m1 > m0:                                   # a span wider than the range needs
                    lo, hi = max(lo - 7, 0), min(hi + 5, T)
                hi = max(hi, lo)
                ref = resample_device(flat[lo:hi].reshape(-1), rate, MODEL_RATE, device=gpu, out_range=(m0, m1), total=T,
                                      first_index=lo, channels=C, channel=ch, src_format=name)
            assert ref.shape == (m1 - m0,)
            fields = dict(src_first_index=lo, src_len=hi - lo, total_len=T, m0=m0, m1=m1,
                          bank_offset=-1 if rate == MODEL_RATE else bank_at[rate], src_format=code, channels=C, channel=chan,
                          o=o, n=n, width=width)
            entries.append((fields, flat[lo:hi].tobytes(), ref))
    order = g.permutation(len(entries))
    entries = [entries[i] for i in order]
    t = Table()
    t.desc = np.zeros(len(entries), dtype=_lib.ingest_desc_dtype())
    stage, tiles, row, at = bytearray(), 0, 0, 3
    for i, (fields, data, ref) in enumerate(entries):
        for k, v in fields.items():
            t.desc[k][i] = v
        count = fields["m1"] - fields["m0"]
        if at + count > ROW:
            row, at = row + 1, 1
        t.desc["src_offset"][i], t.desc["tile0"][i], t.desc["dst_offset"][i] = len(stage), tiles, row * ROW + at
        stage += data + b"\xa5" * (-len(data) % 16)
        tiles += -(-count // 1024)
        at += count + int(g.integers(0, 6))                              # gaps of 0 .. 5 floats: neighbours must not be touched
    assert row < ROWS and len(entries) >= 40 and tiles > len(entries) // 2
    t.refs = [e[2] for e in entries]
    stage += b"\xa5" * 16                                                # (a source moved by one byte stays inside)
    t.stage = torch.from_numpy(np.frombuffer(bytes(stage), dtype=np.uint8).copy()).to(gpu)
    t.banks = torch.cat(banks)
    return t


def fresh_pool(gpu):
    return torch.full((ROWS, ROW), SENTINEL, device=gpu, dtype=torch.float32)


def test_one_launch_gives_the_bits_of_the_single_calls(gpu, table):
    from diarizen_amd import _lib, ops
    assert {int(f) for f in table.desc["src_format"]} == set(range(8))
    pool = fresh_pool(gpu)
    _lib.profile_enable(True)
    try:
        _lib.profile_collect()
        ops.ingest_many(table.stage, table.desc, table.banks, pool)
        torch.cuda.synchronize()
        prof = {e["name"]: e["launches"] for e in _lib.profile_collect()}
    finally:
        _lib.profile_enable(False)
    assert prof.get("ingest_many") == 1 and "resample" not in prof and "decode" not in prof      # ONE launch
    flat = pool.view(-1)
    written = torch.zeros(flat.numel(), dtype=torch.bool, device=gpu)
    for i, ref in enumerate(table.refs):
        a = int(table.desc["dst_offset"][i])
        assert torch.equal(flat[a:a + ref.numel()], ref), (i, table.desc[i])
        assert not written[a:a + ref.numel()].any()
        written[a:a + ref.numel()] = True
    assert bool((flat[~written] == SENTINEL).all())                      # nothing else was touched
    assert int(written.sum()) == sum(r.numel() for r in table.refs)


def test_no_descriptors_and_no_tiles_launch_nothing(gpu, table):
    from diarizen_amd import _lib, ops
    pool = fresh_pool(gpu)
    ops.ingest_many(table.stage, table.desc[:0], table.banks, pool)
    empty = table.desc[(table.desc["m1"] == table.desc["m0"])].copy()
    assert len(empty) >= 2
    empty["tile0"] = 0
    _lib.profile_enable(True)
    try:
        _lib.profile_collect()
        ops.ingest_many(table.stage, empty, table.banks, pool)
        torch.cuda.synchronize()
        assert not [e for e in _lib.profile_collect() if e["name"] == "ingest_many"]
    finally:
        _lib.profile_enable(False)
    assert bool((pool == SENTINEL).all())


def test_refusals_name_the_descriptor_and_launch_nothing(gpu, table):
    from diarizen_amd import ops
    from diarizen_amd._lib import DznError
    d = table.desc
    res = [i for i in range(len(d)) if d["bank_offset"][i] >= 0 and d["m1"][i] - d["m0"][i] > 1]
    s16 = [i for i in range(len(d)) if d["src_format"][i] == 1 and d["m1"][i] > d["m0"][i]]
    multi = [i for i in range(len(d)) if d["channels"][i] > 1 and d["m1"][i] > d["m0"][i]]
    interior = [i for i in res if d["src_first_index"][i] > 0]

    def refused(i, match, **change):
        bad = d.copy()
        for k, v in change.items():
            bad[k][i] = v
        pool = fresh_pool(gpu)
        with pytest.raises(DznError, match=rf"dzn_ingest_many: descriptor {i}: .*{match}"):
            ops.ingest_many(table.stage, bad, table.banks, pool)
        torch.cuda.synchronize()
        assert bool((pool == SENTINEL).all())

    refused(res[0], "src_format 8", src_format=8)
    refused(len(d) - 1, "src_format -1", src_format=-1)
    i = multi[0]
    refused(i, "channel", channel=int(d["channels"][i]))                                  # channel == channels
    refused(i, "channel", channel=-2)
    i = interior[0]
    refused(i, "does not cover", src_first_index=int(d["src_first_index"][i]) + 8)        # the span starts too late
    refused(i, "does not cover", src_len=int(d["src_len"][i]) - 13)                       # ... ends too early
    refused(s16[0], "not aligned to the 2-byte", src_offset=int(d["src_offset"][s16[0]]) + 1)
    i = res[-1]
    refused(i, "reaches past its pool row", dst_offset=(int(d["dst_offset"][i]) // ROW + 1) * ROW - 1)      # one float left in the row
    refused(i, "reaches past its pool row", dst_offset=ROWS * ROW)                        # behind the last row
    refused(i, "leaves the .* bytes of d_stage", src_offset=table.stage.numel() - 1)
    refused(i, "leaves the .* floats of d_banks", bank_offset=table.banks.numel() - 1)
    refused(3, "tile prefix", tile0=int(d["tile0"][3]) + 1)
