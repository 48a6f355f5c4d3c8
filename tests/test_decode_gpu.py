"""dzn_decode (csrc/resample.hip, audio.decode_device) on the MI355X: stored frames -> one float32 channel at the rate they
have.  Every format x channel count x channel choice at the edges of the 256-lane workgroup must be torch.equal to the host
decode (audio._decode_frames, then the channel or audio.downmix), also through a view that starts at frame 1 of a larger
device buffer (an odd byte offset for the 8- and 24-bit forms); then the library's refusals."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from testkit.feeds import stored_forms

pytestmark = pytest.mark.gpu

FRAMES = [1, 255, 256, 257, 1025]      # the block edge of a 256-lane workgroup either side, a ragged multi-block
FORMATS = ["f32", "s16", "u8", "s24", "s32", "ulaw", "alaw"]


@pytest.fixture(scope="module")
def forms():
    """(C, frames) -> stored_forms of frames + 1 frames (the view test drops frame 0); made once"""
    return {(C, T): stored_forms(T + 1, C, seed=100 * C + T) for C in (1, 2, 3) for T in FRAMES}


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("name", FORMATS)
def test_decode_equals_the_host_decode(built_lib, gpu, forms, name, C):
    from diarizen_amd.audio import _decode_frames, decode_device, downmix
    for T in FRAMES:
        stored, dec = forms[(C, T)][name]
        if name in ("ulaw", "alaw") and (T + 1) * C >= 256:
            assert len(np.unique(stored)) == 256                        # all 256 codes
        whole = torch.from_numpy(np.ascontiguousarray(stored).reshape(-1).copy()).to(gpu)
        per_frame = whole.numel() // (T + 1)
        for c in list(range(C)) + ["downmix"]:
            want = downmix(dec) if c == "downmix" else dec[c]
            assert np.array_equal(want, _decode_frames(stored.tobytes(), name, C, c))      # the host decode itself
            got = decode_device(stored[:T], device=gpu, channels=C, channel=c, src_format=name)
            assert got.dtype == torch.float32 and got.shape == (T,)
            assert torch.equal(got.cpu(), torch.from_numpy(want[:T])), (name, C, c, T)
            # frames 1 .. T + 1 through a view of the larger device buffer: byte offset 1 / 3 / ... for u8, G.711 and s24
            view = whole[per_frame:]
            got = decode_device(view, device=gpu, channels=C, channel=c, src_format=name)
            assert torch.equal(got.cpu(), torch.from_numpy(want[1:])), (name, C, c, T, "view")
    if name == "s16":                                                    # the code is inferred for int16
        assert torch.equal(decode_device(stored, device=gpu, channels=C, channel="downmix").cpu(),
                           torch.from_numpy(downmix(dec)))


def test_float32_mono_is_a_copy_and_zero_frames_launch_nothing(built_lib, gpu):
    from diarizen_amd.audio import decode_device
    x = np.random.default_rng(5).standard_normal(1025).astype(np.float32)
    x[:3] = (np.float32("inf"), -0.0, np.float32(1e-42))               # bits, not values
    got = decode_device(x, device=gpu).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    assert decode_device(np.zeros(0, dtype=np.int16), device=gpu, channels=2).shape == (0,)


def test_refusals(built_lib, gpu):
    """format 8, code 0 with two channels, channel -2, channel == channels and a misaligned int16 pointer raise DznError with
    the library's message and launch nothing: the output buffer keeps its bytes and a following valid call still returns"""
    import ctypes as C
    from diarizen_amd import _lib
    from diarizen_amd._lib import DznError
    from diarizen_amd.audio import decode_device
    from testkit.telephony import all_codes
    codes = all_codes(300, 2, seed=3)
    f32 = np.zeros((300, 2), dtype=np.float32)
    with pytest.raises(DznError, match="dzn_decode: src_format 8"):
        decode_device(codes, device=gpu, channels=2, src_format=8)
    with pytest.raises(DznError, match="src_format 0 is float32 mono"):
        decode_device(f32, device=gpu, channels=2, src_format=0)
    with pytest.raises(DznError, match="channel -2 of a source with 2 channel"):
        decode_device(codes, device=gpu, channels=2, channel=-2, src_format="ulaw")
    with pytest.raises(DznError, match="channel 2 of a source with 2 channel"):
        decode_device(codes, device=gpu, channels=2, channel=2, src_format="ulaw")
    with pytest.raises(ValueError, match="uint8 input needs src_format"):
        decode_device(codes, device=gpu, channels=2)
    # an int16 pointer at an odd address: a uint8 buffer viewed from byte 1
    raw = torch.zeros(2 * 64 + 2, dtype=torch.uint8, device=gpu)
    out = torch.full((64,), 7.0, device=gpu)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    rc = lib.dzn_decode(gpu.index, C.c_void_p(raw.data_ptr() + 1), 1, 1, 0, 64, C.c_void_p(out.data_ptr()), st)
    assert rc == -1
    with pytest.raises(DznError, match="not aligned to the 2-byte samples"):
        _lib.check(rc, None, "dzn_decode")
    assert lib.dzn_decode(gpu.index, C.c_void_p(raw.data_ptr() + 2), 4, 1, 0, 16, C.c_void_p(out.data_ptr()), st) == -1   # int32 at +2
    assert lib.dzn_decode(gpu.index, C.c_void_p(raw.data_ptr() + 1), 3, 1, 0, 16, C.c_void_p(out.data_ptr()), st) == 0    # s24: any address
    torch.cuda.synchronize()
    assert torch.equal(out[16:].cpu(), torch.full((48,), 7.0)) and torch.equal(out[:16].cpu(), torch.zeros(16))
    assert decode_device(codes, device=gpu, channels=2, channel=1, src_format="ulaw").shape == (300,)
