"""One handle, many calls: the scripts of tests/_reuse_cases.py played on the device engine.  Nearly every other engine test
creates its handle at exactly (B, N), runs one shape and throws the handle away; production creates one handle at the
largest size and calls it for hours.  Each test plays one script on an OVERSIZE handle (max_batch 6, max_samples 16000)
and `check_script` holds every output to: (a) the bits the same input gave earlier on that handle, before loud audio,
silence and other shapes went through it; (b) the bits of a handle created at exactly the call's size; (c) the float64
oracle at the project's end-to-end bars (fp32 modes 1e-3 and identical decisions outside near ties of the reference,
f16 5e-2 / 99.5 %, embeddings cosine 0.9999 / 0.999); (d) seg_1's bias and the skip counters for windows without an active
speaker; (e) the refusal of a 65th window length with nothing launched; (f) no bit of a window changed by a non-finite
neighbour, in its call or the next (include/dzn.h).  Every equality is exact.  The shipped path only: no environment
switch is set, no debug tap.  test_engine_reuse_host.py shows on a CPU model that these checks catch the mistakes they
are for."""
import ctypes as C

import pytest
import torch

import _reuse_cases as rc

pytestmark = pytest.mark.gpu

_FITS = {}          # (config, precision, with embedding) -> {input id: output of the exact-fit handle}


class _Device:
    """diarizen_amd.engine.Engine behind the interface rc.run_script plays: CPU tensors in, numpy arrays out"""

    def __init__(self, eng, gpu):
        self.eng, self.gpu = eng, gpu

    def segment(self, wave):
        logp, ml, soft = self.eng.segment(wave.to(self.gpu), want_soft=True)
        torch.cuda.synchronize()
        return {"logp": logp.cpu().numpy(), "ml": ml.cpu().numpy(), "soft": soft.cpu().numpy()}

    def embed(self, wave, masks, out=None):
        if out is None:
            emb = self.eng.embed(wave.to(self.gpu), masks.to(self.gpu))
            torch.cuda.synchronize()
            return emb.cpu().numpy()
        # the caller's own output buffer, so that a refused call can be shown to have left it alone
        from diarizen_amd._lib import check
        e, d_wave, d_masks, d_out = self.eng, wave.to(self.gpu), masks.to(self.gpu), out.to(self.gpu)
        (B, N), (_, S, L) = wave.shape, masks.shape
        try:
            check(e.lib.dzn_embed_forward(e._h, C.c_void_p(d_wave.data_ptr()), C.c_void_p(d_masks.data_ptr()), B, S, N, L,
                                          C.c_void_p(d_out.data_ptr()), e._stream()), e._h, "dzn_embed_forward")
        finally:
            torch.cuda.synchronize()
            out.copy_(d_out.cpu())
        return out.numpy()

    def embed_strided(self, rec, B, N, stride, masks):
        views = rec.to(self.gpu).as_strided((B, N), (stride, 1))
        emb = self.eng.embed_strided(views, masks.to(self.gpu))
        torch.cuda.synchronize()
        return emb.cpu().numpy()

    def skip_stats(self):
        torch.cuda.synchronize()
        return self.eng.embed_skip_stats()

    def close(self):
        self.eng.close()


def _play(gpu, script, precision, with_emb):
    from diarizen_amd._lib import DznError
    from diarizen_amd.configs import RESNET34
    from diarizen_amd.engine import Engine
    cfg, sd = rc.get_cfg(script["config"]), rc.seg_weights(script["config"])

    def make(max_batch, max_samples):
        emb = (RESNET34, rc.emb_weights()) if with_emb else (None, None)
        return _Device(Engine(cfg, sd, *emb, max_batch=max_batch, max_samples=max_samples, precision=precision, device=gpu), gpu)
    result = rc.run_script(make, script, _FITS.setdefault((script["config"], precision, with_emb), {}))
    bias = rc.emb_weights()["resnet.seg_1.bias"].numpy() if with_emb else None
    return rc.check_script(script, result, precision, bias=bias, error_type=DznError)


@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("config", rc.SEG_CONFIGS)
def test_seg_history(built_lib, gpu, config, precision):
    """L in {1, 2, 4, 49} and B * L in {1, 2, 126, 128, 129, 294} on one handle, three full-size calls (gain 1e4, digital
    silence, other audio), every shape again in reverse order; each shape also on a handle of exactly its size."""
    _play(gpu, rc.seg_history(config), precision, with_emb=False)


@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_emb_history(built_lib, gpu, precision):
    """T in {8, 9, 17, 98} (stage widths down to 1) at B in {1, 2, 6}, the same three phases; then the shared frame grid
    (melg) alternating with the dense fbank path (fb) at one T, and windows 1 and 4 silent between two calls in which
    they are active (the trunk subset over stale images)."""
    _play(gpu, rc.emb_history(), precision, with_emb=True)


@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_emb_geometries(built_lib, gpu, precision):
    """64 distinct window lengths T = 8 ... 71 on one handle, the 65th refused with its output buffer untouched, then
    T = 8 and T = 71 again with the bits they gave before"""
    _play(gpu, rc.emb_geometries(), precision, with_emb=True)


@pytest.mark.parametrize("precision", rc.PRECISIONS)
@pytest.mark.parametrize("config", rc.SEG_CONFIGS)
def test_seg_poison(built_lib, gpu, config, precision):
    """window 2 of 4 with one NaN sample, one +Inf sample, every sample 3e38: windows 0, 1, 3 keep the clean call's bits
    and the clean call after it equals the clean call before it"""
    _play(gpu, rc.poison("seg", config), precision, with_emb=False)


@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_emb_poison(built_lib, gpu, precision):
    """the same three variants through the fbank, the ResNet trunk and its per-image trackers: the embeddings of windows
    0, 1, 3 keep their bits, and so does the clean call that follows"""
    _play(gpu, rc.poison("emb", rc.EMB_CONFIG), precision, with_emb=True)


def test_attention_planes_ignores_what_lies_past_the_window(built_lib, gpu):
    """What test_seg_poison found in the f32h engine, at the kernel: the last 64-key tile of a window reaches into the next
    window's K / V rows and, behind the batch, into whatever the planes held before.  Those keys' probabilities are exactly
    0, but 0 x NaN = NaN in P'V' put a non-finite neighbour into this window, and its stale planes into the next call.
    L = 49: 15 keys of every tile lie past the window.  Window 0 next to a NaN / Inf window 1, and window 1 in front of
    NaN-filled scratch behind the batch, give the bits they give next to finite data over zeroed scratch."""
    from diarizen_amd import ops
    B, L, h = 2, 49, 2
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * L, 3 * h * 64, generator=g).to(gpu)
    amax = qkv.reshape(B, -1).abs().amax(1).contiguous()
    want = ops.attention_planes(qkv, B, L, h, amax=amax).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    for bad in (float("nan"), float("inf")):
        poisoned = qkv.clone()
        poisoned[L:] = bad                               # every q, k, v of window 1
        got = ops.attention_planes(poisoned, B, L, h, amax=amax)
        torch.cuda.synchronize()
        assert torch.equal(got[:L], want[:L]), f"window 0 changed next to a window of {bad}"
    planes = torch.full((2, B * L + 64, 2 * h * 64), 0x7e00, device=gpu, dtype=torch.int16)        # fp16 NaN in every slot
    kvs = torch.full((B * L + 64, 2 * h), float("nan"), device=gpu)
    got = ops.attention_planes(qkv, B, L, h, amax=amax, planes=planes, kvs=kvs)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "stale non-finite planes behind the batch reached the last window"
