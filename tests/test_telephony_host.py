"""Telephony ingest on the host (diarizen_amd/audio.py): the G.711 tables against `audioop`, A-law / mu-law RIFF/WAVE files,
NIST SPHERE files, the channel choice (an index or "downmix") and `pipeline.open_recording`.  Every comparison is a bit
equality: G.711 expansion is an integer table and the other conversions are multiplications by powers of two."""
from __future__ import annotations

import audioop

import numpy as np
import pytest
import torch

from testkit.telephony import all_codes, sphere_bytes, wav_bytes

RANGES = ((0, 700), (0, 17), (123, 300), (690, 100), (700, 10), (900, 5))      # start, middle, across the end, past it
F = 700                                                                          # frames per file


def _tables():
    from diarizen_amd.audio import alaw_table, ulaw_table
    return {"ulaw": ulaw_table(), "alaw": alaw_table()}


def test_g711_tables_equal_audioop():
    """ulaw_table / alaw_table == audioop.ulaw2lin / alaw2lin on all 256 codes; the ranges and the two zeros of mu-law"""
    t = _tables()
    codes = bytes(range(256))
    for name, ref in (("ulaw", audioop.ulaw2lin), ("alaw", audioop.alaw2lin)):
        want = np.frombuffer(ref(codes, 2), dtype="<i2")
        assert t[name].dtype == np.int16 and t[name].shape == (256,)
        assert np.array_equal(t[name], want), name
    assert t["ulaw"].max() == 32124 and t["ulaw"].min() == -32124 and t["ulaw"][0x7F] == 0 and t["ulaw"][0xFF] == 0
    assert t["alaw"].max() == 32256 and t["alaw"].min() == -32256


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name,tag", [("alaw", 6), ("ulaw", 7)])
def test_g711_wav(tmp_path, name, tag, channels, extensible):
    """tags 6 / 7, plain and WAVE_FORMAT_EXTENSIBLE: load_wav == table[bytes] * 2^-15; WavSource.read == slices of it;
    read_stored == the stored bytes with the format's code; read_raw stays None"""
    from diarizen_amd.audio import SRC_FORMATS, WavSource, load_audio, load_wav
    codes = all_codes(F, channels, seed=tag)
    blob = wav_bytes(tag, channels, 8000, 8, codes.tobytes(), extensible)
    want = (_tables()[name][codes].astype(np.float32) * np.float32(2.0 ** -15)).T
    x, sr = load_wav(blob)
    assert sr == 8000 and x.dtype == np.float32 and np.array_equal(x, want)
    assert np.array_equal(load_audio(blob)[0], want)
    p = tmp_path / "g711.wav"
    p.write_bytes(blob)
    for ch in range(channels):
        src = WavSource(p, channel=ch)
        assert (src.sample_rate, src.channels, src.num_samples) == (8000, channels, F)
        for start, n in RANGES:
            got = src.read(start, n)
            assert got.dtype == np.float32 and np.array_equal(got, want[ch, start:start + n]), (ch, start, n)
            stored, code = src.read_stored(start, n)
            assert code == SRC_FORMATS[name] and stored.dtype == np.uint8
            assert np.array_equal(stored, codes[start:start + n])
        assert src.read_raw(0, 10) is None


def test_read_stored_of_the_pcm_and_float_forms(tmp_path):
    """read_stored: the frames as stored with codes 1 .. 5 (0 for mono float32), None for float64; read_raw is None for
    everything except PCM16"""
    from diarizen_amd.audio import WavSource
    g = np.random.default_rng(5)
    pcm = g.integers(-32768, 32768, size=(F, 2)).astype("<i2")
    u8 = g.integers(0, 256, size=(F, 2)).astype(np.uint8)
    s24 = g.integers(0, 256, size=(F, 6)).astype(np.uint8)
    s32 = g.integers(-2 ** 31, 2 ** 31, size=(F, 2)).astype("<i4")
    f32 = g.standard_normal((F, 2)).astype("<f4")
    files = {"s16": (1, 2, 16, pcm, 1), "u8": (1, 2, 8, u8, 2), "s24": (1, 2, 24, s24, 3), "s32": (1, 2, 32, s32, 4),
             "f32": (3, 2, 32, f32, 5), "f32mono": (3, 1, 32, f32[:, :1], 0), "f64": (3, 2, 64, f32.astype("<f8"), None)}
    for name, (tag, nch, bits, frames, code) in files.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(wav_bytes(tag, nch, 8000, bits, np.ascontiguousarray(frames).tobytes()))
        src = WavSource(p)
        if code is None:
            assert src.read_stored(0, 10) is None
        else:
            for start, n in RANGES:
                stored, c = src.read_stored(start, n)
                assert c == code and stored.dtype == frames.dtype, name
                assert np.array_equal(stored, frames[start:start + n]), (name, start, n)
        raw = src.read_raw(3, 10)
        assert np.array_equal(raw, pcm[3:13]) if name == "s16" else raw is None


SPHERE_CASES = [("pcm", 2, "01", 1, 1024), ("pcm", 2, "10", 2, 1024), (None, 2, "01", 2, 2048), ("ulaw", 1, None, 1, 1024),
                ("ulaw", 1, None, 2, 2048), ("mu-law", 1, None, 2, 1024), ("alaw", 1, None, 1, 2048), ("alaw", 1, None, 2, 1024)]


@pytest.mark.parametrize("coding,n_bytes,order,channels,header", SPHERE_CASES)
def test_sphere(tmp_path, coding, n_bytes, order, channels, header):
    """load_sphere == SphereSource.read == the expected samples: pcm16 of both byte orders (and without a sample_coding
    field), ulaw / mu-law, alaw, 1 and 2 channels, 1024- and 2048-byte headers; load_audio dispatches on NIST_1A"""
    from diarizen_amd.audio import SRC_FORMATS, SphereSource, load_audio, load_sphere
    if n_bytes == 2:
        pcm = np.random.default_rng(header + channels).integers(-32768, 32768, size=(F, channels)).astype(np.int16)
        body = pcm.astype("<i2" if order == "01" else ">i2").tobytes()
        want = (pcm.astype(np.float32) * np.float32(2.0 ** -15)).T
        code, stored_want = (1, pcm) if order == "01" else (None, None)
    else:
        name = "alaw" if coding == "alaw" else "ulaw"
        codes = all_codes(F, channels, seed=header + channels)
        body = codes.tobytes()
        want = (_tables()[name][codes].astype(np.float32) * np.float32(2.0 ** -15)).T
        code, stored_want = SRC_FORMATS[name], codes
    blob = sphere_bytes(coding, channels, 8000, n_bytes, body, byte_format=order, header=header)
    x, sr = load_sphere(blob)
    assert sr == 8000 and x.dtype == np.float32 and x.shape == (channels, F) and np.array_equal(x, want)
    y, sr2 = load_audio(blob)
    assert sr2 == 8000 and np.array_equal(y, want)
    p = tmp_path / "x.sph"
    p.write_bytes(blob)
    assert np.array_equal(load_sphere(str(p))[0], want)
    for ch in range(channels):
        src = SphereSource(p, channel=ch)
        assert (src.sample_rate, src.channels, src.num_samples) == (8000, channels, F)
        for start, n in RANGES:
            got = src.read(start, n)
            assert got.dtype == np.float32 and np.array_equal(got, want[ch, start:start + n]), (ch, start, n)
            stored = src.read_stored(start, n)
            if code is None:
                assert stored is None                       # big-endian PCM16: the device does not take it
            else:
                assert stored[1] == code and np.array_equal(stored[0], stored_want[start:start + n])


def test_sphere_sample_count_beyond_the_data(tmp_path):
    """a sample_count larger than the data present is cut to the data present (and a smaller one cuts the data)"""
    from diarizen_amd.audio import SphereSource, load_sphere
    codes = all_codes(F, 2, seed=9)
    want = (_tables()["ulaw"][codes].astype(np.float32) * np.float32(2.0 ** -15)).T
    for count, frames in ((F + 1000, F), (F - 100, F - 100)):
        blob = sphere_bytes("ulaw", 2, 8000, 1, codes.tobytes(), sample_count=count)
        x, _ = load_sphere(blob)
        assert np.array_equal(x, want[:, :frames])
        p = tmp_path / f"count{count}.sph"
        p.write_bytes(blob)
        src = SphereSource(p, channel=1)
        assert src.num_samples == frames
        assert np.array_equal(src.read(frames - 10, 100), want[1, frames - 10:frames])


def test_sphere_refusals(tmp_path):
    """shorten-compressed files are refused naming SPHERE and shorten; a truncated or zero header naming SPHERE"""
    from diarizen_amd.audio import SphereSource, load_audio, load_sphere
    body = bytes(400)
    short = sphere_bytes("ulaw,embedded-shorten-v2.00", 2, 8000, 1, body)
    good = sphere_bytes("ulaw", 2, 8000, 1, body)
    bad = {"shorten": short, "truncated": good[:300], "zero": b"NIST_1A\n" + bytes(60),
           "no end_head": good[:1024].replace(b"end_head", b"        ") + body,
           "no rate": good.replace(b"sample_rate", b"sample_xxxx"),
           "pcm24": sphere_bytes("pcm", 1, 8000, 3, body, byte_format="01")}
    for name, blob in bad.items():
        match = "(?s)SPHERE.*shorten" if name == "shorten" else "SPHERE"
        with pytest.raises(ValueError, match=match):
            load_sphere(blob)
        with pytest.raises(ValueError, match=match):
            load_audio(blob)
        p = tmp_path / "bad.sph"
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=match):
            SphereSource(p)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_downmix_equals_torch_mean(C):
    """downmix == torch.mean(dim=0) bit for bit for C = 2, 3, 4 on 100 003 seeded normal samples; C = 1: the channel"""
    from diarizen_amd.audio import downmix
    x = np.random.default_rng(100 + C).standard_normal((C, 100003)).astype(np.float32)
    got = downmix(x)
    assert got.dtype == np.float32 and got.shape == (100003,)
    if C == 1:
        assert np.array_equal(got, x[0])
    else:
        assert np.array_equal(got, torch.from_numpy(x).mean(dim=0).numpy())


@pytest.fixture(scope="module")
def call8k(tmp_path_factory):
    """an 8 kHz two-channel mu-law call as WAV and as SPHERE, and its decoded channels float32 [2, F]"""
    codes = all_codes(F, 2, seed=21)
    d = tmp_path_factory.mktemp("telephony")
    (d / "call.wav").write_bytes(wav_bytes(7, 2, 8000, 8, codes.tobytes()))
    (d / "call.sph").write_bytes(sphere_bytes("ulaw", 2, 8000, 1, codes.tobytes()))
    decoded = (_tables()["ulaw"][codes].astype(np.float32) * np.float32(2.0 ** -15)).T
    return str(d / "call.wav"), str(d / "call.sph"), np.ascontiguousarray(decoded)


def test_channel_choice(tmp_path, call8k):
    """first_channel_16k(channel=1) is channel 1, channel="downmix" the mean, each == resample(decoded, 8000, 16000); the
    default stays channel 0; the lazy sources make the same choice; an index >= the channel count is refused"""
    from diarizen_amd.audio import SphereSource, WavSource, downmix, first_channel_16k, resample
    wav, sph, x = call8k
    mean = downmix(x)
    assert np.array_equal(mean, torch.from_numpy(x).mean(dim=0).numpy())
    for path, source in ((wav, WavSource), (sph, SphereSource)):
        assert np.array_equal(first_channel_16k(path, 8000, channel=1), x[1])
        assert np.array_equal(first_channel_16k(path, 8000, channel="downmix"), mean)
        assert np.array_equal(first_channel_16k(path), resample(x[0], 8000, 16000))
        assert np.array_equal(first_channel_16k(path, channel=1), resample(x[1], 8000, 16000))
        assert np.array_equal(first_channel_16k(path, channel="downmix"), resample(mean, 8000, 16000))
        assert len(first_channel_16k(path)) == 2 * F
        assert np.array_equal(source(path, channel="downmix").read(100, 300), mean[100:400])
        assert np.array_equal(source(path).read(0, F), x[0])
        for bad in (2, 7):
            with pytest.raises(ValueError, match=f"channel {bad} of a source with 2"):
                source(path, channel=bad)
            with pytest.raises(ValueError, match=f"channel {bad} of a source with 2"):
                first_channel_16k(path, channel=bad)


def test_open_recording_channel(call8k):
    """open_recording: channel= reaches the host path and the lazy sources, a mapping's "channel" beats the argument, bad
    values and an index >= the file's channel count are refused"""
    from diarizen_amd.audio import SphereSource, WavSource, downmix, resample
    from diarizen_amd.pipeline import open_recording
    wav, sph, x = call8k
    up = [resample(x[0], 8000, 16000), resample(x[1], 8000, 16000)]
    for path, source in ((wav, WavSource), (sph, SphereSource)):
        assert np.array_equal(open_recording(path, 16000), up[0])
        assert np.array_equal(open_recording(path, 16000, channel=1), up[1])
        assert np.array_equal(open_recording({"audio": path, "channel": 1}, 16000, channel=0), up[1])
        assert np.array_equal(open_recording({"audio": path}, 16000, channel=1), up[1])
        assert np.array_equal(open_recording({"audio": path, "channel": "downmix"}, 16000),
                              resample(downmix(x), 8000, 16000))
        with open(path, "rb") as f:
            assert np.array_equal(open_recording(f.read(), 16000, channel=1), up[1])
        src = open_recording(path, 8000, lazy=True, channel=1)               # same rate: a lazy source of that channel
        assert isinstance(src, source) and np.array_equal(src.read(0, F), x[1])
        assert np.array_equal(open_recording(path, 16000, lazy=True, channel=1), up[1])
        for bad in (True, -1, 1.0, "mean", "1", None):
            with pytest.raises(ValueError, match="channel"):
                open_recording(path, 16000, channel=bad)
            if bad is not None:                                              # (None in a mapping: no choice of its own)
                with pytest.raises(ValueError, match="channel"):
                    open_recording({"audio": path, "channel": bad}, 16000)
        assert np.array_equal(open_recording({"audio": path, "channel": None}, 16000, channel=1), up[1])
        for kw in ({}, {"lazy": True}):
            with pytest.raises(ValueError, match="channel 2 of a source with 2"):
                open_recording(path, 16000, channel=2, **kw)
            with pytest.raises(ValueError, match="channel 2 of a source with 2"):
                open_recording(path, 8000, channel=2, **kw)
