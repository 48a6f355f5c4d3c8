"""Audio ingest for the pipeline (replaces `torchaudio.load` at diarizen/pipelines/inference.py:127
and the `Audio` helper of PA/core/io.py for what the hot path needs: WAV, (r5) FLAC or NIST SPHERE in, ONE channel kept —
channel 0 by default, "force to use the SDM data", inference.py:128; `channel=` selects another one or "downmix", the
per-file "channel" key and mono="downmix" of PA/core/io.py:53-54, 205-212, 300-303 — resampled to 16 kHz when the file is at
another rate, as `Audio.downmix_and_resample` does with `torchaudio.functional.resample`, PA/core/io.py:214-218).
torchaudio is not available in this image: RIFF/WAVE (PCM 8/16/24/32, float 32/64, G.711 A-law / mu-law,
WAVE_FORMAT_EXTENSIBLE) and SPHERE (`NIST_1A` header; 16-bit PCM of either byte order, mu-law, A-law; not shorten-compressed:
`load_sphere`, `SphereSource`) are parsed directly with numpy.  G.711 is expanded by the integer tables of ITU-T G.711
(`ulaw_table`, `alaw_table`: pinned to `audioop`; parity of SPHERE / G.711 decoding with torchaudio / sox is UNPINNED here),
and the resampler restates torchaudio's default algorithm
(sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; torchaudio==2.1.1 functional/functional.py
`_get_sinc_resample_kernel` / `_apply_sinc_resample_kernel`).  Parity of the resampler is UNPINNED
(no torchaudio here, no fixture in the reference); tests pin its properties instead.

The resampler exists twice over ONE filter bank (`resample_bank`): `resample`, a strided convolution on the host (the default
everywhere), and `resample_device` (csrc/resample.hip, `dzn_resample`), which turns a span of input samples — float32, or the
interleaved frames of a file as stored (`read_stored` of a source: 8 / 16 / 24 / 32-bit PCM, float32, mu-law, A-law; the
kernel decodes them and selects the channel or downmixes) — into a range of output samples on the GPU, with
the bits of the same slice of a whole-recording call (`resample_input_span` says which input a range reads).
`ResampledSource` wraps a file at another rate on top of it; `pipeline.open_recording(resample="device")` returns one.

Array recordings (2 - 64 microphones) have a channel choice of their own, `Beamform`: GCC-PHAT delays per block
(`beamform_delays_device`, csrc/beamform.hip), smoothed on the host (`smooth_delays`), then the channels aligned and averaged
(`beamform_sum_device`); `BeamformedSource` runs the three over a file span by span, and
`pipeline.open_recording(channel=Beamform(...))` returns one.  `Beamform(causal=True)` replaces the smoothing by
`causal_delays`, which looks at no later block: the form a LIVE array feed takes (`FeedFormat(..., channel=Beamform(causal=True))`,
`beam_ready`, `ArrayFeedPlanner`; csrc/beamform_live.hip tracks the delays on the device), with the offline result of the same
file bit for bit.

Live sources deliver the same stored forms in packets: `FeedFormat` names what a session is fed (`feed_format=`), `feed_ready`
says which output samples are final after R frames, `FeedPlanner` turns chunks of bytes into device calls whose ranges tile
the output (streaming.WaveIngest runs them), and `decode_device` (`dzn_decode`) is the decode without the resampler, for feeds
already at the model's rate.
"""
from __future__ import annotations

import io
from typing import BinaryIO, Optional, Tuple, Union

import numpy as np


_PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # KSDATAFORMAT_SUBTYPE_*: tag + this tail


# src_format codes of dzn_resample (include/dzn.h DZN_SRC_*), by the names resample_device takes
SRC_FORMATS = {"f32": 0, "s16": 1, "u8": 2, "s24": 3, "s32": 4, "f32i": 5, "ulaw": 6, "alaw": 7}
_SRC_DTYPES = {0: "float32", 1: "int16", 2: "uint8", 3: "uint8", 4: "int32", 5: "float32", 6: "uint8", 7: "uint8"}
_SRC_BYTES = {0: 4, 1: 2, 2: 1, 3: 3, 4: 4, 5: 4, 6: 1, 7: 1}


def ulaw_table() -> np.ndarray:
    """int16 [256]: the linear value of every G.711 mu-law code byte (ITU-T G.711; == audioop.ulaw2lin).  Range +-32124;
    0x7F and 0xFF both decode to 0.  The float sample is value * 2^-15, exact."""
    u = ~np.arange(256, dtype=np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw_table() -> np.ndarray:
    """int16 [256]: the linear value of every G.711 A-law code byte (ITU-T G.711; == audioop.alaw2lin).  Range +-32256.
    The float sample is value * 2^-15, exact."""
    a = np.arange(256, dtype=np.int32) ^ 0x55
    e, m = (a >> 4) & 7, a & 0x0F
    t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


_G711_F32 = {"ulaw": ulaw_table().astype(np.float32) * np.float32(2.0 ** -15),
             "alaw": alaw_table().astype(np.float32) * np.float32(2.0 ** -15)}


def downmix(x: np.ndarray) -> np.ndarray:
    """float32 [C, N] -> [N], the mean over the channels, DEFINED as a float32 running sum over the channels in ascending
    order, starting from channel 0, then ONE float32 division by float32(C) (C = 1: the channel itself).  The device resampler
    (csrc/resample.hip, channel -1) computes exactly this.  It is bit-identical to `torch.mean(dim=0)` for C = 2, 3, 4; for
    C >= 5 torch sums in another order and a few samples per 100 k differ in the last bit (multiplying by the reciprocal
    instead of dividing would differ from torch in a third of the samples at C = 3)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        return np.ascontiguousarray(x)
    s = np.array(x[0], dtype=np.float32)
    for c in range(1, x.shape[0]):
        s += x[c]
    if x.shape[0] > 1:
        s /= np.float32(x.shape[0])
    return s


def check_channel(channel):
    """a channel choice is an int >= 0 or "downmix" (returned as is); anything else, a bool included, is a ValueError"""
    if isinstance(channel, str) and channel == "downmix":
        return channel
    if isinstance(channel, (int, np.integer)) and not isinstance(channel, (bool, np.bool_)) and channel >= 0:
        return int(channel)
    raise ValueError(f'channel is an int >= 0 or "downmix", not {channel!r}')


def _check_channel_of(channel, channels: int):
    channel = check_channel(channel)
    if channel != "downmix" and channel >= channels:
        raise ValueError(f"channel {channel} of a source with {channels} channel(s)")
    return channel


def select_channel(x: np.ndarray, channel=0) -> np.ndarray:
    """float32 [C, N] -> [N]: channel `channel` of a decoded file, or its `downmix`; an index >= C is a ValueError"""
    channel = _check_channel_of(channel, x.shape[0])
    return downmix(x) if channel == "downmix" else np.ascontiguousarray(x[channel])


_CODEC_DTYPES = {"u8": np.uint8, "s16": "<i2", "s16be": ">i2", "s32": "<i4", "f32": "<f4", "f64": "<f8", "ulaw": np.uint8,
                 "alaw": np.uint8}
_CODEC_BYTES = {"u8": 1, "s16": 2, "s16be": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8, "ulaw": 1, "alaw": 1}
# the stored form the device resampler takes (None: it goes through `read`)
_CODEC_SRC_FORMAT = {"u8": 2, "s16": 1, "s24": 3, "s32": 4, "f32": 5, "ulaw": 6, "alaw": 7}


def _decode_frames(body, codec: str, nch: int, channel=None) -> np.ndarray:
    """float32 of the interleaved frames in `body` with load_wav's conversions: [m, nch] (channel None), [m] of one channel
    (only that channel is converted), or the `downmix` of the frame"""
    sel = channel if isinstance(channel, int) else slice(None)
    if codec == "s24":
        b3 = np.frombuffer(body, dtype=np.uint8).reshape(-1, nch, 3)[:, sel].astype(np.int32)
        v = b3[..., 0] | (b3[..., 1] << 8) | (b3[..., 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        x = v.astype(np.float32) / 8388608.0
    else:
        raw = np.frombuffer(body, dtype=_CODEC_DTYPES[codec]).reshape(-1, nch)[:, sel]
        if codec == "u8":
            x = (raw.astype(np.float32) - 128.0) / 128.0
        elif codec in ("s16", "s16be"):
            x = raw.astype(np.float32) / 32768.0
        elif codec == "s32":
            x = raw.astype(np.float32) / 2147483648.0
        elif codec in ("ulaw", "alaw"):
            x = _G711_F32[codec][raw]
        else:
            x = raw.astype(np.float32)
    if channel == "downmix":
        x = downmix(x.T)
    return np.ascontiguousarray(x)


class _FrameSource:
    """what WavSource and SphereSource share: ONE channel choice of a file of fixed-size interleaved frames behind a header
    (path, _data_off, _frame bytes per frame, _codec, channels, num_samples, _channel)"""

    def _frames(self, start: int, n: int):
        start = max(0, min(int(start), self.num_samples))
        n = max(0, min(int(n), self.num_samples - start))
        with open(self.path, "rb") as f:
            f.seek(self._data_off + start * self._frame)
            return f.read(n * self._frame)

    def read(self, start: int, n: int) -> np.ndarray:
        """float32 [m] = samples start .. start + n of the channel choice (m < n at the end of the file)"""
        return _decode_frames(self._frames(start, n), self._codec, self.channels, self._channel)

    def read_stored(self, start: int, n: int):
        """(array [m, ...], src_format) = the interleaved frames start .. start + n exactly as they lie in the file, not
        converted, with the format code resample_device / dzn_resample decode them by (m < n at the end of the file): int16
        / int32 / float32 [m, channels], uint8 [m, channels] (8-bit PCM, mu-law, A-law) or uint8 [m, 3 channels] (24-bit).
        None where the device cannot take the format (float64, big-endian PCM16): those go through `read`."""
        fmt = _CODEC_SRC_FORMAT.get(self._codec)
        if fmt is None:
            return None
        if fmt == 5 and self.channels == 1:
            fmt = 0
        dt = np.uint8 if self._codec == "s24" else _CODEC_DTYPES[self._codec]
        return np.frombuffer(self._frames(start, n), dtype=dt).reshape(-1, self._frame // np.dtype(dt).itemsize), fmt


def load_wav(src: Union[str, bytes, BinaryIO, io.BytesIO]) -> Tuple[np.ndarray, int]:
    """-> (float32 [channels, samples] in [-1, 1), sample_rate)  (torchaudio.load semantics).
    RIFF/WAVE is parsed directly: PCM 8 / 16 / 24 / 32 bit, IEEE float 32 / 64, G.711 A-law / mu-law (tags 6 / 7, one byte
    per sample, expanded by alaw_table / ulaw_table) and WAVE_FORMAT_EXTENSIBLE (tag 0xFFFE: the real format is the first
    two bytes of the SubFormat GUID) — everything `torchaudio.load` reads from a .wav; the standard `wave` module refuses
    24-bit extensible, float and G.711 files."""
    if isinstance(src, (bytes, bytearray)):
        data = src
    elif hasattr(src, "read"):
        if hasattr(src, "seek"):
            src.seek(0)
        data = src.read()
    else:
        with open(src, "rb") as f:
            data = f.read()
    if bytes(data[:4]) not in (b"RIFF", b"RF64") or bytes(data[8:12]) != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    view = memoryview(data)        # (slicing `bytes` copies: a 4 h file was copied twice before it was decoded)
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        cid, size = bytes(view[pos:pos + 4]), int.from_bytes(view[pos + 4:pos + 8], "little")
        if cid == b"fmt ":
            fmt = bytes(view[pos + 8:pos + 8 + size])
        elif cid == b"data":
            body = view[pos + 8:] if size in (0, 0xFFFFFFFF) else view[pos + 8:pos + 8 + size]   # streamed files
            break
        pos += 8 + size + (size & 1)
    if fmt is None or body is None or len(fmt) < 16:
        raise ValueError("malformed WAVE file")
    tag = int.from_bytes(fmt[0:2], "little")
    nch = int.from_bytes(fmt[2:4], "little")
    sr = int.from_bytes(fmt[4:8], "little")
    block = int.from_bytes(fmt[12:14], "little")
    bits = int.from_bytes(fmt[14:16], "little")
    if tag == 0xFFFE:                                        # WAVE_FORMAT_EXTENSIBLE
        if len(fmt) < 40 or fmt[26:40] != _PCM_GUID_TAIL:
            raise ValueError("unsupported WAVE_FORMAT_EXTENSIBLE sub-format")
        tag = int.from_bytes(fmt[24:26], "little")
    if nch < 1 or sr < 1:
        raise ValueError("malformed WAVE fmt chunk")
    width = block // nch if block else (bits + 7) // 8      # container bytes per sample
    body = body[:len(body) - len(body) % (width * nch)]
    if tag == 1:                                             # integer PCM
        if width == 1:
            x = (np.frombuffer(body, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        elif width == 2:
            x = np.frombuffer(body, dtype="<i2").astype(np.float32)
            x *= np.float32(1.0 / 32768.0)                   # in place; a power of two, so identical to the division
        elif width == 3:
            b3 = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)
            v = np.where(v & 0x800000, v - 0x1000000, v)
            x = v.astype(np.float32) / 8388608.0
        elif width == 4:
            x = np.frombuffer(body, dtype="<i4").astype(np.float32)
            x *= np.float32(1.0 / 2147483648.0)
        else:
            raise ValueError(f"unsupported PCM width {width}")
    elif tag == 3:                                           # IEEE float
        if width == 4:
            x = np.frombuffer(body, dtype="<f4").astype(np.float32)
        elif width == 8:
            x = np.frombuffer(body, dtype="<f8").astype(np.float32)
        else:
            raise ValueError(f"unsupported float width {width}")
    elif tag in (6, 7) and width == 1:                       # G.711 A-law / mu-law
        x = _G711_F32["alaw" if tag == 6 else "ulaw"][np.frombuffer(body, dtype=np.uint8)]
    else:
        raise ValueError(f"unsupported WAVE format tag {tag} ({bits} bit)")
    if nch == 1:
        return x.reshape(1, -1), sr                              # already [1, samples], contiguous
    return x.reshape(-1, nch).T.copy(), sr


_WAV_CODECS = {(1, 1): "u8", (1, 2): "s16", (1, 3): "s24", (1, 4): "s32", (3, 4): "f32", (3, 8): "f64", (6, 1): "alaw",
               (7, 1): "ulaw"}


class WavSource(_FrameSource):
    """Lazy reader of ONE channel (an index, or "downmix": audio.downmix of the frame) of a RIFF/WAVE file: parses the header, then decodes only the byte range a caller
    asks for — with N ranks sharding one recording (pipeline.device_stage) every rank reads 1/N of the file (+ one
    window of halo) instead of decoding all of it.  Same formats and the same float conversion as
    load_wav(); a source at another rate is decoded whole and resampled on the host unless the caller asks for the device
    resampler (ResampledSource, which reads only the input span of a range)."""

    def __init__(self, path, channel=0):
        self.path = str(path)
        channel = check_channel(channel)
        with open(self.path, "rb") as f:
            head = f.read(12)
            if head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
                raise ValueError("not a RIFF/WAVE file")
            fmt = None
            while True:
                ck = f.read(8)
                if len(ck) < 8:
                    raise ValueError("malformed WAVE file")
                cid, size = ck[:4], int.from_bytes(ck[4:8], "little")
                if cid == b"fmt ":
                    fmt = f.read(size)
                    if size & 1:
                        f.seek(1, 1)
                elif cid == b"data":
                    self._data_off = f.tell()
                    f.seek(0, 2)
                    avail = f.tell() - self._data_off
                    self._data_len = avail if size in (0, 0xFFFFFFFF) else min(size, avail)
                    break
                else:
                    f.seek(size + (size & 1), 1)
        if fmt is None or len(fmt) < 16:
            raise ValueError("malformed WAVE file")
        tag = int.from_bytes(fmt[0:2], "little")
        self.channels = int.from_bytes(fmt[2:4], "little")
        self.sample_rate = int.from_bytes(fmt[4:8], "little")
        block = int.from_bytes(fmt[12:14], "little")
        bits = int.from_bytes(fmt[14:16], "little")
        if tag == 0xFFFE:
            if len(fmt) < 40 or fmt[26:40] != _PCM_GUID_TAIL:
                raise ValueError("unsupported WAVE_FORMAT_EXTENSIBLE sub-format")
            tag = int.from_bytes(fmt[24:26], "little")
        if self.channels < 1 or self.sample_rate < 1:
            raise ValueError("malformed WAVE fmt chunk")
        self._width = block // self.channels if block else (bits + 7) // 8
        self._tag, self._channel = tag, _check_channel_of(channel, self.channels)
        self._codec = _WAV_CODECS.get((tag, self._width))
        if self._codec is None:
            raise ValueError(f"unsupported WAVE format tag {tag} ({bits} bit)")
        self._frame = self._width * self.channels
        self.num_samples = self._data_len // self._frame

    def read_raw(self, start: int, n: int):
        """int16 [m, channels] = the interleaved frames start .. start + n of a PCM16 file as stored, not converted
        (m < n at the end of the file); None for every other format, which goes through `read`"""
        if (self._tag, self._width) != (1, 2):
            return None
        start = max(0, min(int(start), self.num_samples))
        n = max(0, min(int(n), self.num_samples - start))
        with open(self.path, "rb") as f:
            f.seek(self._data_off + start * self._frame)
            return np.fromfile(f, dtype="<i2", count=n * self.channels).reshape(-1, self.channels)


def _sphere_header(head: bytes, avail=None):
    """-> (data offset, codec, channels, sample_rate, sample_count or None) of a NIST SPHERE header: `NIST_1A`, the header
    size on the second line, then `name -type value` lines (-i integer, -r real, -sN a string of N characters) up to
    `end_head`.  `head` holds at least the header (the caller reads 8 bytes more than the first 16 say when it is longer)."""
    def bad(why):
        return ValueError(f"malformed NIST SPHERE header: {why}")
    lines = bytes(head[:16]).split(b"\n")
    if len(lines) < 3 or lines[0] != b"NIST_1A" or not lines[1].strip().isdigit():
        raise bad("no header size on the second line")
    size = int(lines[1])
    if size < 16 or size > len(head):
        raise bad(f"a header of {size} bytes in {len(head)}")
    fields, ended = {}, False
    for line in bytes(head[16:size]).split(b"\n"):
        line = line.strip()
        if line == b"end_head":
            ended = True
            break
        if not line or line.startswith(b";"):
            continue
        parts = line.decode("latin-1").split(None, 2)
        if len(parts) < 3 or not parts[1].startswith("-"):
            raise bad(f"field line {line[:40]!r}")
        fields[parts[0]] = parts[2].strip()
    if not ended:
        raise bad("no end_head")
    try:
        sr, nch = int(fields["sample_rate"]), int(fields["channel_count"])
        width = int(fields["sample_n_bytes"])
        count = int(fields["sample_count"]) if "sample_count" in fields else None
    except (KeyError, ValueError) as e:
        raise bad(f"field {e}") from None
    if sr < 1 or nch < 1 or width < 1 or (count is not None and count < 0):
        raise bad("sample_rate / channel_count / sample_n_bytes / sample_count out of range")
    coding = fields.get("sample_coding", "pcm").lower()
    base, _, suffix = coding.partition(",")
    if suffix.startswith("embedded-shorten"):
        raise ValueError(f"unsupported NIST SPHERE sample_coding {coding!r}: shorten-compressed SPHERE files are not decoded "
                         "(expand them first, e.g. sph2pipe -f wav)")
    order = fields.get("sample_byte_format", "")
    if suffix == "" and base == "pcm" and width == 2 and order in ("01", "10"):
        codec = "s16" if order == "01" else "s16be"
    elif suffix == "" and base in ("ulaw", "mu-law") and width == 1:
        codec = "ulaw"
    elif suffix == "" and base == "alaw" and width == 1:
        codec = "alaw"
    else:
        raise ValueError(f"unsupported NIST SPHERE file: sample_coding {coding!r}, sample_n_bytes {width}, "
                         f"sample_byte_format {order!r} (read: 16-bit pcm 01 / 10, ulaw, alaw)")
    return size, codec, nch, sr, count


def _sphere_header_bytes(first: bytes) -> int:
    """how many bytes the header takes, from the first 16 (1024 when they do not say: _sphere_header then refuses)"""
    lines = bytes(first[:16]).split(b"\n")
    return int(lines[1]) if len(lines) >= 2 and lines[1].strip().isdigit() else 1024


def load_sphere(src: Union[str, bytes, BinaryIO, io.BytesIO]) -> Tuple[np.ndarray, int]:
    """-> (float32 [channels, samples] in [-1, 1), sample_rate) of a NIST SPHERE file (what the LDC telephone corpora ship:
    usually mu-law, 8 kHz, one side of the call per channel).  16-bit PCM of either byte order, mu-law and A-law, channels
    interleaved; a sample_count beyond the data present is cut to the data; shorten-compressed files are refused."""
    data = _read_all(src)
    off, codec, nch, sr, count = _sphere_header(bytes(data[:max(16, _sphere_header_bytes(data[:16]))]))
    frame = _CODEC_BYTES[codec] * nch
    frames = (len(data) - off) // frame
    frames = frames if count is None else min(frames, count)
    x = _decode_frames(memoryview(data)[off:off + frames * frame], codec, nch)
    return np.ascontiguousarray(x.T), sr


class SphereSource(_FrameSource):
    """Lazy reader of ONE channel (an index, or "downmix") of a NIST SPHERE file, with WavSource's interface (.sample_rate,
    .channels, .num_samples, .read, .read_stored): the header is parsed, then only the byte range asked for is read.  Same
    formats and conversions as load_sphere()."""

    def __init__(self, path, channel=0):
        self.path = str(path)
        channel = check_channel(channel)
        with open(self.path, "rb") as f:
            first = f.read(16)
            if not first.startswith(b"NIST_1A"):
                raise ValueError("not a NIST SPHERE file")
            head = first + f.read(max(0, _sphere_header_bytes(first) - 16))
            f.seek(0, 2)
            size = f.tell()
        self._data_off, self._codec, self.channels, self.sample_rate, count = _sphere_header(head)
        self._channel = _check_channel_of(channel, self.channels)
        self._frame = _CODEC_BYTES[self._codec] * self.channels
        frames = max(0, size - self._data_off) // self._frame
        self.num_samples = frames if count is None else min(frames, count)


def resample_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """-> (kernels float32 [n, K], o, n, width): the polyphase filter bank of `resample` (torchaudio's
    `_get_sinc_resample_kernel`), o = orig / gcd, n = new / gcd, K = 2 width + o; built in float64, cast to float32.
    Output sample m = f n + p is  sum_j kernels[p, j] x[f o + j - width]  (x = 0 outside the recording)."""
    import math
    import torch
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)
    return kernels.to(torch.float32)[:, 0].numpy(), o, n, width             # [n, 2 width + o]


def resample_ratio(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """-> (o, n, width) of resample_bank, without building the bank (n K float64 values: 2 GB for 15999 Hz -> 16 kHz)"""
    import math
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    return o, n, math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff))


def resample_input_span(m0: int, m1: int, o: int, n: int, width: int):
    """-> (lo, hi): the half-open range of input indices that the output samples [m0, m1) read (see resample_bank); it may
    extend below 0 or beyond the recording, where the input counts as zero.  An empty output range reads nothing."""
    m0, m1 = int(m0), int(m1)
    if m1 <= m0:
        return 0, 0
    return (m0 // n) * o - width, ((m1 - 1) // n) * o + width + o


def feed_ready(frames: int, o: int, n: int, width: int) -> int:
    """the feed schedule of a live source: with `frames` = R input frames of a recording received so far (its end unknown),
    the output samples [0, ready) are FINAL — every tap of theirs lies in [0, R), so they are the samples of the
    whole-recording resample whatever follows — and sample `ready` reads a frame that has not arrived:

        ready(R) = max(0, (R - width) // o) * n

    (resample_input_span(0, ready)[1] <= R < resample_input_span(ready, ready + 1)[1]).  Output lags the feed by at most
    width + o - 1 frames, and a later call still needs fewer than K = 2 width + o of the frames received (`feed_history`)."""
    return max(0, (int(frames) - width) // o) * n


def feed_history(ready: int, o: int, n: int, width: int) -> int:
    """the first input frame that output samples >= `ready` (a value of feed_ready) still read: frames before it can go"""
    return max(0, (int(ready) // n) * o - width)


def resample(x: np.ndarray, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
             rolloff: float = 0.99) -> np.ndarray:
    """float32 [..., T] -> [..., ceil(T * new / orig)]: band-limited sinc interpolation with a Hann
    window, evaluated as one strided convolution with `new/gcd` polyphase filters (torchaudio's default
    `functional.resample`).  The filter bank is built in float64 and applied in float32, like torchaudio."""
    import math
    import torch
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq == new_freq:
        return np.ascontiguousarray(x, dtype=np.float32)
    bank, o, n, width = resample_bank(orig_freq, new_freq, lowpass_filter_width, rolloff)
    kernels = torch.from_numpy(bank)[:, None]                            # [n, 1, 2 width + o]
    w = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    shape = w.shape
    w = w.reshape(-1, shape[-1])
    length = w.shape[-1]
    w = torch.nn.functional.pad(w, (width, width + o))
    y = torch.nn.functional.conv1d(w[:, None], kernels, stride=o)        # [B, n, frames]
    y = y.transpose(1, 2).reshape(w.shape[0], -1)
    target = math.ceil(n * length / o)
    return y[..., :target].reshape(shape[:-1] + (target,)).numpy()


def resampled_length(num_samples: int, o: int, n: int) -> int:
    """ceil(n T / o): the output length of `resample` for T input samples"""
    return -((-n * int(num_samples)) // o)


_DEVICE_BANKS: dict = {}


def _device_bank(orig_freq: int, new_freq: int, device):
    """the filter bank on `device`, tap-major ([K, n]: what dzn_resample reads), uploaded once per (orig, new, device)"""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(orig_freq), int(new_freq), str(device))
    hit = _DEVICE_BANKS.get(key)
    if hit is None:
        bank, o, n, width = resample_bank(orig_freq, new_freq)
        hit = (torch.from_numpy(np.ascontiguousarray(bank.T)).to(device), o, n, width)
        _DEVICE_BANKS[key] = hit
    return hit


def resample_tile() -> int:
    """output samples per workgroup of the device resampler (csrc/resample.hip)"""
    from . import _lib
    return int(_lib.load().dzn_resample_tile())


def _src_format_code(torch_dtype, src_format, channels: int, what: str) -> int:
    """the DZN_SRC_* code of `src_format` (a name of SRC_FORMATS, a code, or None: inferred for float32 mono and int16) for
    input of `torch_dtype`; `what` names the caller in the refusals"""
    dtype = str(torch_dtype).replace("torch.", "")
    if src_format is None:
        if dtype == "int16":
            fmt = 1
        elif dtype == "float32":
            fmt = 0
            if channels != 1:
                raise ValueError(f'{what}: float32 input is mono (interleaved float32 frames: src_format="f32")')
        elif dtype == "uint8":
            raise ValueError(f'{what}: uint8 input needs src_format ("u8", "s24", "ulaw" or "alaw")')
        else:
            raise ValueError(f"{what}: float32 or int16 input, or a src_format, not {torch_dtype}")
    elif isinstance(src_format, str):
        if src_format not in SRC_FORMATS:
            raise ValueError(f"{what}: src_format is one of {sorted(SRC_FORMATS)}, not {src_format!r}")
        fmt = SRC_FORMATS[src_format]
        if fmt == 0 and channels != 1:
            fmt = 5
    else:
        fmt = int(src_format)                              # a code of dzn.h; the library refuses what it does not know
    if fmt in _SRC_DTYPES and dtype != _SRC_DTYPES[fmt]:
        raise ValueError(f"{what}: src_format {src_format!r} is stored as {_SRC_DTYPES[fmt]}, not {torch_dtype}")
    return fmt


def resample_device(x, orig_freq: int, new_freq: int, *, device, out_range=None, total=None, first_index: int = 0,
                    channels: int = 1, channel=0, src_format=None):
    """`resample` on the device (csrc/resample.hip, one launch on the current stream) -> float32 device tensor [m1 - m0].
    x: a host array or a device tensor holding the frames as a file stores them, interleaved over `channels` (flat or
    [frames, ...]); the kernel decodes them and reads `channel` — an index, or "downmix" (audio.downmix of every frame).
    src_format names the stored form (SRC_FORMATS): "f32" (mono, or interleaved when channels > 1: "f32i"), "s16" (sample * 2^-15: what load_wav
    makes of it), "u8" (offset binary), "s24" (uint8 input, 3 bytes per sample, little-endian), "s32", "ulaw", "alaw"
    (uint8 input, G.711) — or the integer code of include/dzn.h.  It is inferred for float32 mono and int16 input and
    required for uint8 input, which is ambiguous.  x holds the frames first_index .. first_index + frames of a recording of `total` samples (default: x is the whole recording);
    out_range = (m0, m1) selects the output samples (default: all ceil(n total / o)); x must cover
    resample_input_span(m0, m1, ...) inside [0, total) (the library refuses otherwise).  A range call returns the bits of the
    same slice of a whole-recording call, and a stored-format call the bits of the float32 call on the host-decoded channel
    (or host downmix).  The result differs from the host `resample` in the last bits (another order of the same float32
    sums)."""
    import ctypes as C
    import torch
    from . import _lib
    device = torch.device(device)
    channels = int(channels)
    if isinstance(x, torch.Tensor):
        xd = x.to(device)
    else:
        x = np.ascontiguousarray(x)
        xd = torch.from_numpy(x if x.flags.writeable else x.copy()).to(device)      # (torch refuses read-only arrays)
    fmt = _src_format_code(xd.dtype, src_format, channels, "resample_device")
    # "downmix" is the library's channel -1; an integer goes to the library as it is, which refuses one out of range
    channel = -1 if isinstance(channel, (str, bool)) and check_channel(channel) == "downmix" else int(channel)
    xd = xd.contiguous().reshape(-1)
    per_frame = max(1, channels) * (_SRC_BYTES.get(fmt, xd.element_size()) // xd.element_size())
    if xd.numel() % per_frame:
        raise ValueError("resample_device: the input is not a whole number of frames")
    frames = xd.numel() // per_frame
    total = frames + int(first_index) if total is None else int(total)
    bank, o, n, width = _device_bank(orig_freq, new_freq, device)
    m0, m1 = (0, resampled_length(total, o, n)) if out_range is None else (int(out_range[0]), int(out_range[1]))
    out = torch.empty(max(0, m1 - m0), device=device, dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    dev = device.index if device.index is not None else -1
    _lib.check(_lib.load().dzn_resample(dev, C.c_void_p(xd.data_ptr()), fmt, channels, channel, int(first_index),
                                        frames, total, C.c_void_p(bank.data_ptr()), o, n, width, m0, m1,
                                        C.c_void_p(out.data_ptr()), st), None, "dzn_resample")
    return out


class ResampledSource:
    """A recording at another rate, resampled on the device range by range: wraps a WavSource or SphereSource (the frames are
    uploaded as the file stores them — `read_stored`: PCM of 8 / 16 / 24 / 32 bit, float32, mu-law, A-law — and the kernel
    decodes them and applies the source's channel choice; float64 and big-endian files are decoded by `.read` on the host) or
    a decoded one-channel float32 array (`orig_rate` says its rate).  `.sample_rate` is the new rate, `.num_samples` =
    ceil(n T / o) as `resample` gives, and
    `.read_device(start, n)` reads only resample_input_span of the range, uploads it and resamples it: the bits of the same
    slice of read_device(0, num_samples), so every rank of a sharded run touches only the span of its windows."""

    def __init__(self, src, new_rate: int, device, orig_rate: Optional[int] = None):
        self.src, self.device = src, "cuda" if device is None else device      # None: the current HIP device
        self._array = not hasattr(src, "read_stored")
        if self._array:
            if orig_rate is None:
                raise ValueError("ResampledSource: a decoded array needs orig_rate")
            self.src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
            self.orig_rate, self._total = int(orig_rate), len(self.src)
        else:
            self.orig_rate, self._total = int(src.sample_rate), int(src.num_samples)
        self.sample_rate = int(new_rate)
        if self.orig_rate == self.sample_rate:
            raise ValueError("ResampledSource: the source is already at the requested rate")
        _, self._o, self._n, self._width = resample_bank(self.orig_rate, self.sample_rate)
        self.num_samples = resampled_length(self._total, self._o, self._n)

    def read_device(self, start: int, n: int):
        """float32 device tensor [m] = output samples start .. start + n (m < n at the end of the recording)"""
        m0 = max(0, min(int(start), self.num_samples))
        m1 = max(m0, min(m0 + int(n), self.num_samples))
        lo, hi = resample_input_span(m0, m1, self._o, self._n, self._width)
        lo, hi = max(lo, 0), max(min(hi, self._total), 0)
        hi = max(hi, lo)
        kw = dict(device=self.device, out_range=(m0, m1), total=self._total, first_index=lo)
        if self._array:
            return resample_device(self.src[lo:hi], self.orig_rate, self.sample_rate, **kw)
        stored = self.src.read_stored(lo, hi - lo)
        if stored is not None:
            return resample_device(stored[0], self.orig_rate, self.sample_rate, channels=self.src.channels,
                                   channel=self.src._channel, src_format=stored[1], **kw)
        return resample_device(self.src.read(lo, hi - lo), self.orig_rate, self.sample_rate, **kw)


def decode_device(x, *, device, channels: int = 1, channel=0, src_format=None):
    """the decode half of `resample_device` on its own (csrc/resample.hip, `dzn_decode`: one launch on the current stream) ->
    float32 device tensor [frames]: channel `channel` (an index, or "downmix") of the frames in x, a host array or device
    tensor holding them as a file stores them, at the rate they have.  src_format as resample_device takes it.  The result is
    the bits of the host decode (`_decode_frames`, then `select_channel` or `downmix`)."""
    import ctypes as C
    import torch
    from . import _lib
    device = torch.device(device)
    channels = int(channels)
    if isinstance(x, torch.Tensor):
        xd = x.to(device)
    else:
        x = np.ascontiguousarray(x)
        xd = torch.from_numpy(x if x.flags.writeable else x.copy()).to(device)
    fmt = _src_format_code(xd.dtype, src_format, channels, "decode_device")
    channel = -1 if isinstance(channel, (str, bool)) and check_channel(channel) == "downmix" else int(channel)
    xd = xd.contiguous().reshape(-1)
    per_frame = max(1, channels) * (_SRC_BYTES.get(fmt, xd.element_size()) // xd.element_size())
    if xd.numel() % per_frame:
        raise ValueError("decode_device: the input is not a whole number of frames")
    frames = xd.numel() // per_frame
    out = torch.empty(frames, device=device, dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    dev = device.index if device.index is not None else -1
    _lib.check(_lib.load().dzn_decode(dev, C.c_void_p(xd.data_ptr()), fmt, channels, channel, frames,
                                      C.c_void_p(out.data_ptr()), st), None, "dzn_decode")
    return out


# ----------------------------------------------------------------------------- array recordings: GCC-PHAT delay-and-sum
class Beamform:
    """A channel choice for array recordings (`channel=Beamform(...)` where an index or "downmix" is accepted on the offline
    path): the channels are aligned to channel `reference` by per-block time differences of arrival (GCC-PHAT) and averaged
    (csrc/beamform.hip).  max_delay: the search range in seconds (10 ms covers an aperture of about 3.4 m);
    hop: the block hop in samples at the FILE's rate, a power of two in [256, 4096] (default: the largest one <= 0.256 s,
    capped at 4096); min_peak: the GCC-PHAT peak below which a block's delay is not trusted (default 8 / sqrt(2 hop): for
    unrelated channels the correlation is roughly Gaussian with sigma = 1 / sqrt(2 hop), so this is 8 sigma — a statistical
    derivation that no real array recording has met yet).  causal=True replaces the smoothing of the raw delays by the rule
    that looks at no later block (`causal_delays`, DESIGN.md §4.24: a change of delay takes effect two blocks late) — the form a
    live feed takes (`FeedFormat(..., channel=Beamform(causal=True))`), offered offline too so that the live result equals the
    file's.  Validated here; `plan` settles what depends on the file."""

    def __init__(self, reference: int = 0, max_delay: float = 0.01, hop: Optional[int] = None,
                 min_peak: Optional[float] = None, causal: bool = False):
        if isinstance(reference, (bool, np.bool_)) or not isinstance(reference, (int, np.integer)) or reference < 0:
            raise ValueError(f"Beamform: reference is a channel index >= 0, not {reference!r}")
        if isinstance(max_delay, (bool, str)) or not np.isfinite(max_delay) or not max_delay > 0:
            raise ValueError(f"Beamform: max_delay is a positive number of seconds, not {max_delay!r}")
        if hop is not None and (isinstance(hop, (bool, np.bool_)) or not isinstance(hop, (int, np.integer))
                                or hop < 256 or hop > 4096 or hop & (hop - 1)):
            raise ValueError(f"Beamform: hop is a power of two in [256, 4096], not {hop!r}")
        if min_peak is not None and (isinstance(min_peak, (bool, str)) or not np.isfinite(min_peak) or min_peak < 0):
            raise ValueError(f"Beamform: min_peak is a number >= 0, not {min_peak!r}")
        if not isinstance(causal, (bool, np.bool_)):
            raise ValueError(f"Beamform: causal is True or False, not {causal!r}")
        self.causal = bool(causal)
        self.reference, self.max_delay = int(reference), float(max_delay)
        self.hop = None if hop is None else int(hop)
        self.min_peak = None if min_peak is None else float(min_peak)

    def plan(self, rate: int, channels: int) -> Tuple[int, int, float]:
        """-> (hop, max_lag, min_peak) for a file of `channels` channels at `rate` Hz; ValueError for a file with one channel,
        with more than 64, or without the reference channel"""
        rate, channels = int(rate), int(channels)
        if channels < 2 or channels > 64:
            raise ValueError(f"Beamform: a source with {channels} channel(s) (an array has 2 .. 64)")
        if self.reference >= channels:
            raise ValueError(f"Beamform: reference channel {self.reference} of a source with {channels} channel(s)")
        hop = self.hop
        if hop is None:
            hop = 256
            while hop < 4096 and 2 * hop <= 0.256 * rate:
                hop *= 2
        max_lag = min(max(1, int(round(self.max_delay * rate))), hop // 2)
        min_peak = 8.0 / float(np.sqrt(2.0 * hop)) if self.min_peak is None else self.min_peak
        return hop, max_lag, min_peak

    def _key(self):
        return (self.reference, self.max_delay, self.hop, self.min_peak, self.causal)

    def __eq__(self, other):
        return isinstance(other, Beamform) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"Beamform(reference={self.reference}, max_delay={self.max_delay}, hop={self.hop}, "
                f"min_peak={self.min_peak}{', causal=True' if self.causal else ''})")


def beamform_blocks(total: int, hop: int) -> int:
    """ceil(T / hop) + 1: the blocks of a recording of T samples (centres at b hop, frames of 2 hop)"""
    return -(-int(total) // int(hop)) + 1


def beamform_twiddle(hop: int) -> np.ndarray:
    """float32 [hop, 2] = (cos, -sin)(2 pi k / W) for k < W / 2 = hop: computed in float64, rounded once (what
    dzn_beamform_delays takes as d_twiddle; its Hann window comes from the cosines)"""
    a = 2.0 * np.pi * np.arange(int(hop), dtype=np.float64) / (2.0 * int(hop))
    return np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32)


def smooth_delays(lag, peak, total: int, hop: int, min_peak: float, reference: int = 0) -> np.ndarray:
    """raw GCC-PHAT lags int [C, nb] and peaks float32 [C, nb] of a recording of `total` samples -> int32 [C, nb], the delays
    the alignment pass applies.  A block is reliable when its frame holds at least `hop` samples of the recording (a ragged
    last frame of a few samples gives high, meaningless peaks) and its peak >= float32(min_peak).  Every block takes the lag of
    the latest reliable block at or before it, the blocks before the first reliable one take that one's, and a channel without
    any reliable block stays 0; then a median of 5 with mirror padding that does not repeat the edge sample
    (numpy.pad(mode="reflect")) removes isolated outliers (skipped when nb < 3).  The reference row is 0."""
    lag = np.asarray(lag)
    peak = np.asarray(peak, dtype=np.float32)
    C, nb = lag.shape
    total, hop = int(total), int(hop)
    if nb != beamform_blocks(total, hop) or peak.shape != lag.shape:
        raise ValueError(f"smooth_delays: [C, {beamform_blocks(total, hop)}] lags and peaks for {total} samples at hop {hop}, "
                         f"not {lag.shape} / {peak.shape}")
    b = np.arange(nb, dtype=np.int64)
    support = np.minimum(total, (b + 1) * hop) - np.maximum(0, (b - 1) * hop) >= hop
    out = np.zeros((C, nb), dtype=np.int32)
    for c in range(C):
        if c == reference:
            continue
        reliable = support & (peak[c] >= np.float32(min_peak))
        if not reliable.any():
            continue
        at = np.maximum.accumulate(np.where(reliable, b, -1))
        at[at < 0] = np.argmax(reliable)
        held = lag[c][at].astype(np.int64)
        if nb >= 3:
            padded = np.pad(held, 2, mode="reflect")
            held = np.median(np.stack([padded[k:k + nb] for k in range(5)]), axis=0)
        out[c] = held.astype(np.int32)
    return out


def causal_delays(lag, peak, total: int, hop: int, min_peak: float, reference: int = 0) -> np.ndarray:
    """`smooth_delays` restated so that delay[c, b] depends on blocks <= b alone (what a live feed can know; the device form
    is dzn_beamform_track, csrc/beamform_live.hip): same arguments -> int32 [C, nb].  A block is reliable as in `smooth_delays`
    (its frame holds at least `hop` samples of the recording, its peak >= float32(min_peak)); held[b] = lag[c, b] if reliable,
    else held[b - 1], with held[-1] = 0 — no backward fill: a channel aligns from its first reliable block on; delay[c, b] = the
    median of held[b - 4 .. b] with held[k] = held[0] for k < 0, a trailing median of 5 whose left edge repeats the first
    entry.  The reference row is 0.  A change of delay takes effect two blocks late."""
    lag = np.asarray(lag)
    peak = np.asarray(peak, dtype=np.float32)
    C, nb = lag.shape
    total, hop = int(total), int(hop)
    if nb != beamform_blocks(total, hop) or peak.shape != lag.shape:
        raise ValueError(f"causal_delays: [C, {beamform_blocks(total, hop)}] lags and peaks for {total} samples at hop {hop}, "
                         f"not {lag.shape} / {peak.shape}")
    b = np.arange(nb, dtype=np.int64)
    support = np.minimum(total, (b + 1) * hop) - np.maximum(0, (b - 1) * hop) >= hop
    out = np.zeros((C, nb), dtype=np.int32)
    for c in range(C):
        if c == reference:
            continue
        reliable = support & (peak[c] >= np.float32(min_peak))
        at = np.maximum.accumulate(np.where(reliable, b, -1))       # the latest reliable block at or before b, -1: none yet
        held = np.where(at >= 0, lag[c][np.maximum(at, 0)], 0).astype(np.int64)
        padded = np.concatenate([np.full(4, held[0], dtype=np.int64), held])
        out[c] = np.median(np.stack([padded[k:k + nb] for k in range(5)]), axis=0).astype(np.int32)
    return out


def beam_ready(frames: int, hop: int) -> int:
    """the schedule of an array feed: with `frames` = R frames received (the end unknown), nc = R // hop blocks are complete
    and the beamformed samples [0, max(0, nc - 1) hop) are FINAL — sample n of block b reads n + delay of blocks b and b + 1,
    below (b + 2) hop.  Output lags the feed by less than 2 hop frames."""
    return max(0, int(frames) // int(hop) - 1) * int(hop)


_DEVICE_TWIDDLES: dict = {}


def _device_twiddle(hop: int, device):
    """beamform_twiddle(hop) on `device`, uploaded once per (hop, device)"""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(hop), str(device))
    hit = _DEVICE_TWIDDLES.get(key)
    if hit is None:
        hit = _DEVICE_TWIDDLES[key] = torch.from_numpy(beamform_twiddle(hop)).to(device)
    return hit


def beamform_tile() -> int:
    """output samples per workgroup of the alignment pass (csrc/beamform.hip)"""
    from . import _lib
    return int(_lib.load().dzn_beamform_tile())


def beamform_delays_span(b0: int, b1: int, hop: int, total: int):
    """-> (lo, hi): the samples of the recording that the frames of blocks [b0, b1) hold"""
    if b1 <= b0:
        return 0, 0
    lo, hi = max(0, (int(b0) - 1) * hop), min(int(total), int(b1) * hop)
    return lo, max(lo, hi)


def beamform_sum_span(delays, hop: int, n0: int, n1: int, total: int):
    """-> (lo, hi): the hull of the samples inside [0, total) that output samples [n0, n1) read with `delays` int [C, nb]
    (sample n of block b reads n + delay of blocks b and b + 1 in every channel); (0, 0) when they read nothing"""
    n0, n1, hop, total = int(n0), int(n1), int(hop), int(total)
    if n1 <= n0:
        return 0, 0
    d = np.asarray(delays, dtype=np.int64)
    ba, bz = n0 // hop, (n1 - 1) // hop + 1                      # the last block used is bz
    b = np.arange(ba, bz, dtype=np.int64)
    s0, s1 = np.maximum(n0, b * hop), np.minimum(n1, (b + 1) * hop)
    pair = np.stack([d[:, ba:bz], d[:, ba + 1:bz + 1]], axis=2)   # [C, blocks, 2]
    a = np.maximum(0, s0[None, :, None] + pair)
    z = np.minimum(total, s1[None, :, None] + pair)
    ok = a < z
    if not ok.any():
        return 0, 0
    return int(a[ok].min()), int(z[ok].max())


def _planar_on_device(x, device):
    """float32 [C, len] on `device`, contiguous, from a host array or a tensor"""
    import torch
    if isinstance(x, torch.Tensor):
        xd = x.to(device=device, dtype=torch.float32)
    else:
        x = np.ascontiguousarray(x, dtype=np.float32)
        xd = torch.from_numpy(x if x.flags.writeable else x.copy()).to(device)
    if xd.dim() != 2:
        raise ValueError(f"planar float32 [channels, samples], not a tensor of shape {tuple(xd.shape)}")
    return xd.contiguous()


def beamform_delays_device(x, *, device, reference: int, hop: int, max_lag: int, total=None, first_index: int = 0,
                           blocks=None):
    """raw GCC-PHAT delays on the device (csrc/beamform.hip, `dzn_beamform_delays`: one launch on the current stream) ->
    (lag int32 [C, b1 - b0], peak float32 [C, b1 - b0]) device tensors for blocks = (b0, b1) (default: all ceil(T / hop) + 1).
    x: planar float32 [C, len], a host array or device tensor, holding samples first_index .. first_index + len of a recording
    of `total` samples (default: x is the whole recording); it must cover beamform_delays_span(b0, b1, hop, total) (the
    library refuses otherwise).  A range call returns the bits of the same columns of a whole-recording call."""
    import ctypes as C
    import torch
    from . import _lib
    device = torch.device(device)
    xd = _planar_on_device(x, device)
    channels, length = int(xd.shape[0]), int(xd.shape[1])
    total = length + int(first_index) if total is None else int(total)
    hop = int(hop)
    if hop < 256 or hop > 4096 or hop & (hop - 1):          # (the twiddle table is built for it before the library sees it)
        raise ValueError(f"beamform_delays_device: hop is a power of two in [256, 4096], not {hop}")
    b0, b1 = (0, beamform_blocks(total, hop)) if blocks is None else (int(blocks[0]), int(blocks[1]))
    lag = torch.empty((channels, max(0, b1 - b0)), device=device, dtype=torch.int32)
    peak = torch.empty((channels, max(0, b1 - b0)), device=device, dtype=torch.float32)
    tw = _device_twiddle(hop, device)
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    dev = device.index if device.index is not None else -1
    _lib.check(_lib.load().dzn_beamform_delays(dev, C.c_void_p(xd.data_ptr()), channels, length, int(first_index), length,
                                               total, int(reference), int(hop), int(max_lag), C.c_void_p(tw.data_ptr()),
                                               b0, b1, C.c_void_p(lag.data_ptr()), C.c_void_p(peak.data_ptr()), st),
               None, "dzn_beamform_delays")
    return lag, peak


def beamform_sum_device(x, delays, *, device, hop: int, total=None, first_index: int = 0, out_range=None, out=None):
    """the alignment pass on the device (csrc/beamform.hip, `dzn_beamform_sum`) -> float32 device tensor [n1 - n0] for
    out_range = (n0, n1) (default: the whole recording).  x as beamform_delays_device takes it; it must cover
    beamform_sum_span(delays, hop, n0, n1, total).  delays: int [C, nb] of the WHOLE recording (smooth_delays), a host array or
    an int32 device tensor.  The call waits for the delays on the current stream (the library checks the columns it uses on the
    host), then enqueues one launch.  The result is bit for bit the float32 restatement (testkit/beamform_ref.py: synth)."""
    import ctypes as C
    import torch
    from . import _lib
    device = torch.device(device)
    xd = _planar_on_device(x, device)
    channels, length = int(xd.shape[0]), int(xd.shape[1])
    total = length + int(first_index) if total is None else int(total)
    if isinstance(delays, torch.Tensor):
        dd = delays.to(device=device, dtype=torch.int32).contiguous()
    else:
        dd = torch.from_numpy(np.ascontiguousarray(delays, dtype=np.int32)).to(device)
    if dd.dim() != 2 or dd.shape[0] != channels:
        raise ValueError(f"beamform_sum_device: delays [{channels}, blocks], not {tuple(dd.shape)}")
    n0, n1 = (0, total) if out_range is None else (int(out_range[0]), int(out_range[1]))
    if out is None:
        out = torch.empty(max(0, n1 - n0), device=device, dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    dev = device.index if device.index is not None else -1
    _lib.check(_lib.load().dzn_beamform_sum(dev, C.c_void_p(xd.data_ptr()), channels, length, int(first_index), length, total,
                                            int(hop), C.c_void_p(dd.data_ptr()), int(dd.shape[1]), n0, n1,
                                            C.c_void_p(out.data_ptr()), st), None, "dzn_beamform_sum")
    return out


class BeamformedSource:
    """An array recording reduced to one channel on the device (`open_recording(..., channel=Beamform(...))`): wraps a
    WavSource or SphereSource — the frames are uploaded as the file stores them (`read_stored`) and made planar float32 by
    `dzn_decode`, one call per channel; forms the device does not decode go through the host decode — or a decoded float32
    [C, T] array (`orig_rate` says its rate).  `.sample_rate` is `new_rate`, `.num_samples` the length at that rate, and
    `.read_device(start, n)` returns the bits of the same slice of read_device(0, num_samples).

    The first read estimates the delays of the whole recording: blocks go to `dzn_beamform_delays` in spans of about SPAN
    frames plus a halo of one hop, the [C, nb] lags and peaks come back (`.lags`, `.peaks`: raw) and `smooth_delays` makes
    `.delays` of them (`causal_delays` for a Beamform(causal=True)).  Every read then walks its range in spans of at most SPAN samples, uploads the frames a span reads
    (beamform_sum_span: a halo of at most hop / 2) and runs `dzn_beamform_sum`, so a 4 h, 8-channel file is never on the
    device as a whole.  A file at another rate than `new_rate` is beamformed at ITS rate and then resampled by the device
    resampler (csrc/resample.hip), whatever `resample=` says: the samples are already on the device."""

    SPAN = 1 << 22

    def __init__(self, src, new_rate: int, device, beamform: Beamform, orig_rate: Optional[int] = None):
        if not isinstance(beamform, Beamform):
            raise ValueError(f"BeamformedSource: beamform is an audio.Beamform, not {beamform!r}")
        self.src, self.device, self.beamform = src, "cuda" if device is None else device, beamform
        self._array = not hasattr(src, "read_stored")
        if self._array:
            if orig_rate is None:
                raise ValueError("BeamformedSource: a decoded array needs orig_rate")
            self.src = np.asarray(src, dtype=np.float32)
            if self.src.ndim != 2:
                raise ValueError("BeamformedSource: a decoded array is float32 [channels, samples]")
            self.orig_rate, self.channels, self._total = int(orig_rate), int(self.src.shape[0]), int(self.src.shape[1])
        else:
            self.orig_rate, self.channels, self._total = int(src.sample_rate), int(src.channels), int(src.num_samples)
        self.hop, self.max_lag, self.min_peak = beamform.plan(self.orig_rate, self.channels)
        self.num_blocks = beamform_blocks(self._total, self.hop)
        self.sample_rate = int(new_rate)
        if self.orig_rate == self.sample_rate:
            self._o = self._n = 1
            self._width = 0
            self.num_samples = self._total
        else:
            self._o, self._n, self._width = resample_ratio(self.orig_rate, self.sample_rate)
            self.num_samples = resampled_length(self._total, self._o, self._n)
        self.lags = self.peaks = self.delays = None
        self._d_delays = None

    def _planar(self, lo: int, hi: int):
        """float32 device tensor [C, hi - lo] = samples lo .. hi of every channel"""
        import ctypes as C
        import torch
        from . import _lib
        device = torch.device(self.device)
        if self._array:
            return _planar_on_device(self.src[:, lo:hi], device)
        stored = self.src.read_stored(lo, hi - lo) if hi > lo else None
        if stored is None:          # nothing to read, or a form only the host decodes (float64, big-endian PCM16)
            x = _decode_frames(self.src._frames(lo, hi - lo), self.src._codec, self.channels)
            return _planar_on_device(x.reshape(-1, self.channels).T, device)
        arr, fmt = stored
        raw = torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(device).reshape(-1)
        frames = int(arr.shape[0])
        out = torch.empty((self.channels, frames), device=device, dtype=torch.float32)
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        dev = device.index if device.index is not None else -1
        lib = _lib.load()
        for c in range(self.channels):
            _lib.check(lib.dzn_decode(dev, C.c_void_p(raw.data_ptr()), fmt, self.channels, c, frames,
                                      C.c_void_p(out[c].data_ptr()), st), None, "dzn_decode")
        return out

    def estimate(self):
        """the delays of the whole recording (done once; the first read calls it) -> `.delays` int32 [C, nb]"""
        import torch
        if self.delays is not None:
            return self.delays
        per = max(1, self.SPAN // self.hop)
        lags, peaks = [], []
        for b0 in range(0, self.num_blocks, per):
            b1 = min(self.num_blocks, b0 + per)
            lo, hi = beamform_delays_span(b0, b1, self.hop, self._total)
            lag, peak = beamform_delays_device(self._planar(lo, hi), device=self.device, reference=self.beamform.reference,
                                               hop=self.hop, max_lag=self.max_lag, total=self._total, first_index=lo,
                                               blocks=(b0, b1))
            lags.append(lag.cpu().numpy())
            peaks.append(peak.cpu().numpy())
        self.lags, self.peaks = np.concatenate(lags, axis=1), np.concatenate(peaks, axis=1)
        rule = causal_delays if self.beamform.causal else smooth_delays
        self.delays = rule(self.lags, self.peaks, self._total, self.hop, self.min_peak, self.beamform.reference)
        self._d_delays = torch.from_numpy(self.delays).to(self.device)
        return self.delays

    def _beam(self, n0: int, n1: int, out=None):
        """float32 device tensor [n1 - n0]: the beamformed samples n0 .. n1 at the file's rate"""
        lo, hi = beamform_sum_span(self.delays, self.hop, n0, n1, self._total)
        return beamform_sum_device(self._planar(lo, hi), self._d_delays, device=self.device, hop=self.hop, total=self._total,
                                   first_index=lo, out_range=(n0, n1), out=out)

    def read_device(self, start: int, n: int):
        """float32 device tensor [m] = output samples start .. start + n (m < n at the end of the recording)"""
        import torch
        m0 = max(0, min(int(start), self.num_samples))
        m1 = max(m0, min(m0 + int(n), self.num_samples))
        self.estimate()
        out = torch.empty(m1 - m0, device=self.device, dtype=torch.float32)
        if self.orig_rate == self.sample_rate:
            for a in range(m0, m1, self.SPAN):
                z = min(m1, a + self.SPAN)
                self._beam(a, z, out=out[a - m0:z - m0])
            return out
        step = max(1, self.SPAN * self._n // self._o)
        for a in range(m0, m1, step):
            z = min(m1, a + step)
            lo, hi = resample_input_span(a, z, self._o, self._n, self._width)
            lo, hi = max(lo, 0), max(min(hi, self._total), 0)
            hi = max(hi, lo)
            out[a - m0:z - m0] = resample_device(self._beam(lo, hi), self.orig_rate, self.sample_rate, device=self.device,
                                                 out_range=(a, z), total=self._total, first_index=lo)
        return out


# ----------------------------------------------------------------------------- live feeds in a stored format
class FeedFormat:
    """What a live source delivers to a session (`feed_format=` of pipeline.stream / open_live / stream_live and of the
    detection pipelines' open_stream / stream): interleaved frames of `channels` samples at `rate` Hz, little-endian, in
    `encoding` — a key of SRC_FORMATS: "f32", "s16", "u8", "s24", "s32", "ulaw", "alaw" (G.711, one byte per sample).
    `channel` is the channel the session hears: an index, "downmix" (audio.downmix of every frame), a
    Beamform(causal=True) for a microphone array (2 .. 64 channels: GCC-PHAT delay-and-sum inside the device ingest,
    `ArrayFeedPlanner`), or None for the pipeline's own `channel`.  A phone call is FeedFormat(8000, "ulaw", channels=2,
    channel=...), a microphone FeedFormat(48000, "s16"), a meeting-room array FeedFormat(16000, "s16", channels=8,
    channel=Beamform(causal=True)).  A bad encoding, a channel the frames do not have, an array geometry Beamform.plan refuses
    and a Beamform that is not causal are refused here."""

    def __init__(self, rate: int, encoding: str, channels: int = 1, channel=None):
        if not isinstance(encoding, str) or encoding not in SRC_FORMATS:
            raise ValueError(f"FeedFormat: encoding is one of {sorted(SRC_FORMATS)}, not {encoding!r}")
        if isinstance(rate, bool) or int(rate) != rate or rate < 1:
            raise ValueError(f"FeedFormat: rate is a positive integer, not {rate!r}")
        if isinstance(channels, bool) or int(channels) != channels or channels < 1:
            raise ValueError(f"FeedFormat: channels is a positive integer, not {channels!r}")
        self.rate, self.encoding, self.channels = int(rate), encoding, int(channels)
        if isinstance(channel, Beamform):
            if not channel.causal:
                raise ValueError(f"FeedFormat: channel={channel!r} is not causal, and a live feed cannot look at later blocks: "
                                 "pass Beamform(causal=True)")
            channel.plan(self.rate, self.channels)                              # refuses 1 or > 64 channels, a missing reference
            self.channel = channel
        else:
            self.channel = None if channel is None else _check_channel_of(channel, self.channels)
        code = SRC_FORMATS[encoding]
        self.src_format = 5 if code == 0 and self.channels != 1 else code       # float32 frames of several channels: "f32i"
        self.dtype = np.dtype(_SRC_DTYPES[code])                                # of an array fed to the session
        self.frame_bytes = _SRC_BYTES[code] * self.channels

    def with_channel(self, channel) -> "FeedFormat":
        """this format with its channel choice settled: its own, or `channel` where it has none"""
        return FeedFormat(self.rate, self.encoding, self.channels, channel if self.channel is None else self.channel)

    def channel_code(self) -> int:
        """the channel as dzn_resample / dzn_decode take it (-1: downmix); an array feed has none"""
        if isinstance(self.channel, Beamform):
            raise ValueError("FeedFormat: an array feed (channel=Beamform) has no channel code")
        return -1 if self.channel == "downmix" else int(self.channel)

    def __repr__(self):
        return f"FeedFormat({self.rate}, {self.encoding!r}, channels={self.channels}, channel={self.channel!r})"


def resample_tile_fits(o: int, n: int, width: int, tile: int) -> bool:
    """whether the input of one tile of `tile` output samples fits the 64 KiB of LDS the device resampler stages it in
    (dzn_resample refuses the ratio otherwise; even o: one pad word per 32)"""
    span = ((tile - 1) // n + 1) * o + 2 * width + o
    floats = span if o & 1 else span + (span >> 5) + 1
    return 4 * floats <= 64 * 1024


class FeedCall:
    """one planned device call of a live feed: `data` = the stored frames first .. first + frames of the recording (the
    history a range still reads, then new frames), `total` = frames received when the call is made (its total_len), and
    [m0, m1) the output samples it makes — by dzn_resample, or by dzn_decode when the feed is at the model's rate (then
    first = m0 and frames = m1 - m0)"""
    __slots__ = ("data", "first", "frames", "total", "m0", "m1")

    def __init__(self, data, first: int, frames: int, total: int, m0: int, m1: int):
        self.data, self.first, self.frames, self.total, self.m0, self.m1 = data, first, frames, total, m0, m1


class FeedPlanner:
    """The host half of a stored-format feed (streaming.WaveIngest runs its calls; needs no device): turns chunks of bytes of
    any length into FeedCalls whose ranges tile the output [0, ceil(n T / o)) exactly once and in order.

    After R frames the samples below feed_ready(R) are final.  A chunk may end inside a frame (the remainder is carried and
    dropped at the end of the stream, as the file readers do with size // frame); the frames a later range still reads —
    fewer than K = 2 width + o, from feed_history(ready) on — are kept here as raw bytes and go in front of the next upload,
    so nothing survives a call on the device.  A chunk of more than `slot_frames` new frames is split; an upload is at most
    K - 1 + slot_frames frames.  `finish()` is the one call with the true length: [ready, ceil(n R / o)), zero tail on the
    right.  A feed at the model's rate is decoded, not resampled: ready = R, no history."""

    def __init__(self, fmt: FeedFormat, model_rate: int, slot_frames: int):
        self.fmt, self.model_rate = fmt, int(model_rate)
        self.same_rate = fmt.rate == self.model_rate
        if self.same_rate:
            self.o, self.n, self.width = 1, 1, 0
        else:
            self.o, self.n, self.width = resample_ratio(fmt.rate, self.model_rate)
        self.K = 2 * self.width + self.o
        self.slot_frames = int(slot_frames)
        if self.slot_frames < 1:
            raise ValueError("FeedPlanner: a slot holds at least one frame")
        self.max_upload_frames = self.slot_frames + (0 if self.same_rate else self.K - 1)
        self.frames = 0                                                 # R: whole frames received
        self.ready = 0                                                  # output samples planned so far: [0, ready) is final
        self.finished = False
        self._partial = b""                                             # the bytes of a frame that has not ended
        self._hist = b""                                                # frames _hist_first .. R as stored
        self._hist_first = 0

    def length_after(self, nbytes: int) -> int:
        """the output length if the stream ended after `nbytes` more bytes"""
        return resampled_length(self.frames + (len(self._partial) + nbytes) // self.fmt.frame_bytes, self.o, self.n)

    def append(self, data) -> list:
        """data: bytes-like, or an array of the format's stored dtype -> the calls that the new frames make possible"""
        if self.finished:
            raise RuntimeError("feed already finished")
        fb = self.fmt.frame_bytes
        buf = self._partial + _feed_bytes(data, self.fmt)
        whole = len(buf) // fb
        self._partial = buf[whole * fb:]
        calls = []
        for f0 in range(0, whole, self.slot_frames):
            k = min(self.slot_frames, whole - f0)
            self._hist += buf[f0 * fb:(f0 + k) * fb]
            self.frames += k
            ready = feed_ready(self.frames, self.o, self.n, self.width)
            if ready > self.ready:
                calls.append(self._call(ready))
        return calls

    def finish(self) -> list:
        """end of stream: a trailing partial frame is dropped; -> the call for [ready, ceil(n R / o)), if any"""
        if self.finished:
            return []
        self.finished, self._partial = True, b""
        total = resampled_length(self.frames, self.o, self.n)
        return [self._call(total)] if total > self.ready else []

    def _call(self, ready: int) -> FeedCall:
        call = FeedCall(self._hist, self._hist_first, self.frames - self._hist_first, self.frames, self.ready, ready)
        self.ready = ready
        keep = self.frames if self.same_rate else feed_history(ready, self.o, self.n, self.width)
        self._hist = self._hist[(keep - self._hist_first) * self.fmt.frame_bytes:]
        self._hist_first = keep
        return call


class ArrayFeedCall:
    """one planned device call of an array feed (dzn_beamform_feed, then dzn_resample where the rates differ): `data` = the
    stored frames first .. first + frames (history, then new frames), `total` = frames received when the call is made (the
    true length at the end of the stream), [b0, b1) the blocks it completes, [n0, n1) the beamformed samples it makes at the
    feed's rate, and [m0, m1) the model-rate samples — equal to [n0, n1) for a feed at the model's rate; otherwise resampled
    from the beamformed samples s_first .. n1, of which [s_first, n0) are carried over from the call before"""
    __slots__ = ("data", "first", "frames", "total", "b0", "b1", "n0", "n1", "s_first", "m0", "m1")

    def __init__(self, data, first, frames, total, b0, b1, n0, n1, s_first, m0, m1):
        self.data, self.first, self.frames, self.total = data, first, frames, total
        self.b0, self.b1, self.n0, self.n1, self.s_first, self.m0, self.m1 = b0, b1, n0, n1, s_first, m0, m1


class ArrayFeedPlanner:
    """The host half of an array feed, `FeedFormat(..., channel=Beamform(causal=True))` (streaming.WaveIngest runs its calls;
    needs no device): turns chunks of bytes of any length into ArrayFeedCalls whose sample ranges tile [0, T) exactly once and
    in order at the feed's rate, and whose block ranges tile the ceil(T / hop) + 1 blocks.

    After R frames nc = R // hop blocks are complete and the samples below beam_ready(R) are final; a call is planned whenever
    nc grows.  A chunk may end inside a frame (the remainder is carried and dropped at the end of the stream).  The frames a
    later call still reads — from max(0, (nc - 1) hop - max_lag) on — are kept here as raw bytes and go in front of the next
    upload, so no samples survive a call on the device; a chunk of more than `slot_frames` new frames is split, and an upload is
    at most slot_frames + 2 hop + max_lag frames.  `finish()` is the one call with the true length: the remaining blocks and
    [ready, T).  Where the feed's rate differs from the model's, the beamformed signal is the source of the device resampler
    with FeedPlanner's arithmetic, "frames received" replaced by `ready` (T at finish): `out_ready` model-rate samples are
    final, and a call names the first beamformed sample (`s_first`) its resample range still reads."""

    def __init__(self, fmt: FeedFormat, model_rate: int, slot_frames: int):
        if not isinstance(fmt.channel, Beamform):
            raise ValueError(f"ArrayFeedPlanner: a FeedFormat with channel=Beamform(causal=True), not {fmt!r}")
        self.fmt, self.model_rate = fmt, int(model_rate)
        self.beamform = fmt.channel
        self.hop, self.max_lag, self.min_peak = fmt.channel.plan(fmt.rate, fmt.channels)
        self.same_rate = fmt.rate == self.model_rate
        if self.same_rate:
            self.o, self.n, self.width = 1, 1, 0
        else:
            self.o, self.n, self.width = resample_ratio(fmt.rate, self.model_rate)
        self.K = 2 * self.width + self.o
        self.slot_frames = int(slot_frames)
        if self.slot_frames < 1:
            raise ValueError("ArrayFeedPlanner: a slot holds at least one frame")
        H = self.hop
        self.max_upload_frames = self.slot_frames + 2 * H + self.max_lag
        self.max_blocks = max(2, (self.slot_frames + H - 1) // H)        # blocks one call completes at the most
        self.max_new = self.max_blocks * H                              # beamformed samples one call makes at the most
        self.frames = 0                                                 # R: whole frames received
        self.blocks = 0                                                 # blocks planned so far (nc; every block once finished)
        self.ready = 0                                                  # beamformed samples planned so far: [0, ready) is final
        self.out_ready = 0                                              # model-rate samples planned so far
        self.finished = False
        self._partial = b""
        self._hist = b""                                                # frames _hist_first .. R as stored
        self._hist_first = 0

    def length_after(self, nbytes: int) -> int:
        """the output length if the stream ended after `nbytes` more bytes"""
        return resampled_length(self.frames + (len(self._partial) + nbytes) // self.fmt.frame_bytes, self.o, self.n)

    def append(self, data) -> list:
        """data: bytes-like, or an array of the format's stored dtype -> the calls that the new frames make possible"""
        if self.finished:
            raise RuntimeError("feed already finished")
        fb = self.fmt.frame_bytes
        buf = self._partial + _feed_bytes(data, self.fmt)
        whole = len(buf) // fb
        self._partial = buf[whole * fb:]
        calls = []
        for f0 in range(0, whole, self.slot_frames):
            k = min(self.slot_frames, whole - f0)
            self._hist += buf[f0 * fb:(f0 + k) * fb]
            self.frames += k
            nc = self.frames // self.hop
            if nc > self.blocks:
                calls.append(self._call(nc, beam_ready(self.frames, self.hop), False))
        return calls

    def finish(self) -> list:
        """end of stream: a trailing partial frame is dropped; -> the call for the remaining blocks and [ready, T)"""
        if self.finished:
            return []
        self.finished, self._partial = True, b""
        return [self._call(beamform_blocks(self.frames, self.hop), self.frames, True)]

    def _call(self, blocks: int, ready: int, last: bool) -> ArrayFeedCall:
        if self.same_rate:
            s_first, out = self.ready, ready
        else:
            s_first = feed_history(self.out_ready, self.o, self.n, self.width)
            out = resampled_length(ready, self.o, self.n) if last else feed_ready(ready, self.o, self.n, self.width)
            out = max(out, self.out_ready)
        call = ArrayFeedCall(self._hist, self._hist_first, self.frames - self._hist_first, self.frames, self.blocks, blocks,
                             self.ready, ready, min(s_first, self.ready), self.out_ready, out)
        self.blocks, self.ready, self.out_ready = blocks, ready, out
        keep = max(self._hist_first, max(0, (blocks - 1) * self.hop - self.max_lag))
        self._hist = self._hist[(keep - self._hist_first) * self.fmt.frame_bytes:]
        self._hist_first = keep
        return call


def _feed_bytes(data, fmt: FeedFormat) -> bytes:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    a = np.asarray(data)
    if a.dtype != fmt.dtype:
        raise ValueError(f"a {fmt.encoding} feed takes bytes or {fmt.dtype} arrays, not {a.dtype}")
    return np.ascontiguousarray(a).tobytes()


def _read_all(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return src
    if hasattr(src, "read"):
        if hasattr(src, "seek"):
            src.seek(0)
        return src.read()
    with open(src, "rb") as f:
        return f.read()


def load_flac(src: Union[str, bytes, BinaryIO, io.BytesIO], verify_md5: bool = True) -> Tuple[np.ndarray, int]:
    """-> (float32 [channels, samples] in [-1, 1), sample_rate) of a FLAC stream (torchaudio.load semantics: integer samples
    divided by 2^(bits - 1)).  Decoded by the native decoder of libdzn_hip.so (csrc/flac.cpp: host code, written from the
    format specification — libFLAC / libsndfile / torchaudio are not in this image); frame CRCs are verified inside, and the
    STREAMINFO MD5 of the decoded PCM here (a stream whose MD5 field is set cannot decode to wrong samples silently)."""
    import ctypes as C
    import hashlib
    from . import _lib
    data = bytes(_read_all(src))
    lib = _lib.load()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    sr, ch, bits, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    md5 = (C.c_uint8 * 16)()
    rc = lib.dzn_flac_info(buf, len(data), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(total), md5)
    if rc != 0:
        raise ValueError("not a FLAC stream (or a malformed STREAMINFO block)")
    # Output capacity.  A frame is at least 11 bytes (header 5 + one CONSTANT subframe + CRC-16) and carries at most 65535
    # samples per channel, so a stream of len(data) bytes cannot hold more than `bound` samples: a STREAMINFO total beyond it
    # is a lie (36-bit field: up to 2^36 samples = a multi-TB allocation before any frame is checked) and is refused.  A stream
    # of unknown length (total 0: piped encoders) starts from 4 samples per byte and doubles on DZN_E_NOMEM up to the bound -
    # digital silence codes 4096 samples in ~10 bytes, so a fixed guess would call a valid file corrupt.
    bound = (len(data) // 11 + 1) * 65535
    if total.value > bound:
        raise ValueError(f"FLAC STREAMINFO claims {total.value} samples, a {len(data)}-byte stream holds at most {bound}")
    cap = total.value if total.value > 0 else max(4096, len(data) * 4)
    done = C.c_int64()
    while True:
        out = np.empty((cap, ch.value), dtype=np.int32)
        rc = lib.dzn_flac_decode(buf, len(data), out.ctypes.data_as(C.c_void_p), cap, C.byref(done))
        if rc == -2 and total.value == 0 and cap < bound:      # DZN_E_NOMEM (include/dzn.h): capacity too small
            cap = min(cap * 2, bound)
            continue
        break
    if rc != 0:
        raise ValueError(f"FLAC decode failed (code {rc}): corrupt frame (CRC / syntax) or an unsupported stream")
    out = out[:done.value]
    if verify_md5 and any(md5):
        width = (bits.value + 7) // 8
        if width == 4:
            raw = out.astype("<i4").tobytes()
        else:
            raw = out.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes()      # little-endian, sign already extended
        if hashlib.md5(raw).digest() != bytes(md5):
            raise ValueError("FLAC decode: MD5 of the decoded samples differs from the STREAMINFO signature")
    x = out.T.astype(np.float32) * np.float32(1.0 / float(1 << (bits.value - 1)))
    return np.ascontiguousarray(x), sr.value


_FORMATS = ((b"fLaC", "FLAC"), (b"OggS", "Ogg (Vorbis / Opus / FLAC-in-Ogg)"), (b"ID3", "MP3 (ID3 tag)"), (b"\xff\xfb", "MP3"),
            (b"\xff\xf3", "MP3"), (b"\xff\xf2", "MP3"), (b"FORM", "AIFF"), (b".snd", "Sun AU"), (b"\x1aE\xdf\xa3", "Matroska / WebM"))


def load_audio(src) -> Tuple[np.ndarray, int]:
    """`torchaudio.load` for what this image can decode natively: RIFF/WAVE (load_wav), FLAC (load_flac) and NIST SPHERE
    (load_sphere).  Anything else is
    refused BY NAME (the reference accepts whatever torchaudio's backend reads, diarizen/pipelines/inference.py:127; here an
    unsupported container must not surface as "not a RIFF/WAVE file")."""
    data = _read_all(src)
    head = bytes(data[:12])
    if head[:4] in (b"RIFF", b"RF64"):
        return load_wav(data)
    if head[:4] == b"fLaC":
        return load_flac(data)
    if head.startswith(b"NIST_1A"):
        return load_sphere(data)
    if len(head) >= 8 and head[4:8] == b"ftyp":
        raise ValueError("unsupported audio container: MP4 / M4A (AAC) — decodable formats: WAV, FLAC, SPHERE")
    for magic, name in _FORMATS:
        if head.startswith(magic):
            raise ValueError(f"unsupported audio format: {name} — decodable formats: WAV (PCM / float / G.711), FLAC, SPHERE")
    raise ValueError("unrecognised audio file (decodable formats: WAV (PCM / float / G.711), FLAC, SPHERE)")


def first_channel_16k(src, expected_sr: int = 16000, channel=0) -> np.ndarray:
    """-> float32 [N] at `expected_sr`: channel 0 of the file (inference.py:128) — or channel `channel`, or the `downmix` of
    its channels (PA/core/io.py:205-212) — resampled if needed."""
    x, sr = load_audio(src)
    x0 = select_channel(x, channel)
    if sr != expected_sr:
        x0 = resample(x0, sr, expected_sr)
    return x0
