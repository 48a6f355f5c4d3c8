// resample.hip — the polyphase sinc resampler of the ingest path on the device (dzn_resample; torchaudio's
// functional.resample as Audio.downmix_and_resample calls it, PA/core/io.py:214-218; the host form is audio.resample).
//
//   y[m] = sum_{j < K} bank[p][j] * x[f o + j - width],   m = f n + p,  K = 2 width + o,  x = 0 outside [0, T)
//
// One workgroup makes kResampleTile consecutive output samples.  It stages the input samples they read — ((tile - 1) / n + 1) o
// + K at most — in LDS, decoding the frames as the file stores them (stored_sample: int16 * 2^-15, 8 / 24 / 32-bit PCM, G.711
// mu-law / A-law by their integer expansion; one channel of the frame or its downmix) and zero-filling outside the recording,
// then every lane walks the K taps of its output sample with ONE fp32 accumulator: acc = fmaf(tap_j, x_j, acc) for
// j = 0 .. K-1.  That order depends on m alone, not on the tile, the lane, the requested range or the stored format, so a
// range call gives the bits of the same slice of a whole-recording call, and a stored-format call the bits of the float32
// call on the host-decoded channel.  The format is a template parameter: the staging loop is the only code that differs.
//
// Lanes hold consecutive m.  The bank is tap-major ([K][n]), so the taps of a wavefront are one coalesced read (n > 1: p runs
// with the lane) or a wave-uniform scalar read (n == 1).  The LDS reads of a wavefront are o floats apart for every n lanes
// (n lanes share a frame and broadcast): conflict-free for odd o; for even o (32 kHz -> 16 kHz: o = 2) the image carries one
// pad word per 32, which spreads the lanes of a 32-lane group over all 32 banks again.  The bank itself is not staged
// (44.1 kHz: 160 x 475 floats = 304 KB): it stays in L2.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(resample)

#include "resample_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

template <int FMT, bool PAD>
__global__ __launch_bounds__(kThreads) void resample_kernel(const void* __restrict__ src, int channels, int channel,
                                                            int64_t src_first, int64_t src_len, int64_t T,
                                                            const float* __restrict__ bank, int o, int n, int width, int K,
                                                            int64_t m0, int64_t m1, float* __restrict__ dst, int lds_floats) {
  extern __shared__ float xs[];
  resample_tile<FMT, PAD>(src, channels, channel, src_first, src_len, T, bank, o, n, width, K, m0, m1, dst, blockIdx.x,
                          lds_floats, xs);
}

// dzn_decode: the staging loop of resample_kernel on its own, for a source that is already at the model's rate (the bank for
// equal rates is a low-pass, not the identity, so the resampler cannot serve it).  One stored frame per lane, consecutive
// lanes on consecutive frames; the downmix is the same running sum and ONE division.  No LDS, nothing tuned: a live chunk is
// a few KB and the call is launch-bound.
template <int FMT>
__global__ __launch_bounds__(kThreads) void decode_kernel(const void* __restrict__ src, int channels, int channel,
                                                          int64_t frames, float* __restrict__ dst) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= frames) return;
  decode_frame<FMT>(src, channels, channel, frames, r, dst);
}

}  // namespace

int launch_decode(const void* src, int format, int channels, int channel, int64_t frames, float* dst, hipStream_t st) {
  if (frames < 0 || format < 0 || format >= DZN_SRC_FORMATS) return DZN_E_INVALID;
  if (frames == 0) return DZN_OK;
  const int64_t blocks = cdiv64(frames, kThreads);
  if (blocks > 0x7fffffff) return DZN_E_INVALID;
  ProfScope prof_scope_(st, "decode", 0.0, (double)frames * (kFormatBytes[format] * channels + 4.0));
  const dim3 grid((unsigned)blocks), block(kThreads);
#define DZN_DECODE_FORMAT(FMT)                                                                            \
  case FMT:                                                                                               \
    hipLaunchKernelGGL((decode_kernel<FMT>), grid, block, 0, st, src, channels, channel, frames, dst);    \
    break
  switch (format) {
    DZN_DECODE_FORMAT(DZN_SRC_F32);
    DZN_DECODE_FORMAT(DZN_SRC_S16);
    DZN_DECODE_FORMAT(DZN_SRC_U8);
    DZN_DECODE_FORMAT(DZN_SRC_S24);
    DZN_DECODE_FORMAT(DZN_SRC_S32);
    DZN_DECODE_FORMAT(DZN_SRC_F32I);
    DZN_DECODE_FORMAT(DZN_SRC_ULAW);
    DZN_DECODE_FORMAT(DZN_SRC_ALAW);
  }
#undef DZN_DECODE_FORMAT
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int32_t dzn_resample_tile(void) { return kResampleTile; }

// the LDS image of the widest tile: 0 when it does not fit (the caller refuses the ratio)
size_t resample_lds_bytes(int o, int n, int width) {
  const int64_t span = ((int64_t)(kResampleTile - 1) / n + 1) * o + 2 * (int64_t)width + o;
  const int64_t floats = (o & 1) ? span : span + (span >> 5) + 1;
  const size_t bytes = (size_t)floats * sizeof(float);
  return bytes <= kMaxLds ? bytes : 0;
}

int launch_resample(const void* src, int format, int channels, int channel, int64_t src_first, int64_t src_len, int64_t T,
                    const float* bank, int o, int n, int width, int64_t m0, int64_t m1, float* dst, hipStream_t st) {
  const size_t lds = resample_lds_bytes(o, n, width);
  if (!lds || m1 < m0 || format < 0 || format >= DZN_SRC_FORMATS) return DZN_E_INVALID;
  if (m1 == m0) return DZN_OK;
  const int K = 2 * width + o;
  const int64_t blocks = cdiv64(m1 - m0, kResampleTile);
  if (blocks > 0x7fffffff) return DZN_E_INVALID;
  const double in_samples = (double)(m1 - m0) * o / n;
  ProfScope prof_scope_(st, "resample", 2.0 * (double)(m1 - m0) * K,
                        in_samples * kFormatBytes[format] * channels + 4.0 * (double)(m1 - m0));
  const dim3 grid((unsigned)blocks), block(kThreads);
  const int lds_floats = (int)(lds / sizeof(float));
#define DZN_RESAMPLE_LAUNCH(FMT, PAD)                                                                                  \
  hipLaunchKernelGGL((resample_kernel<FMT, PAD>), grid, block, lds, st, src, channels, channel, src_first, src_len, T, \
                     bank, o, n, width, K, m0, m1, dst, lds_floats)
#define DZN_RESAMPLE_FORMAT(FMT)                                                          \
  case FMT:                                                                               \
    if (pad) DZN_RESAMPLE_LAUNCH(FMT, true); else DZN_RESAMPLE_LAUNCH(FMT, false);        \
    break
  const bool pad = !(o & 1);
  switch (format) {
    DZN_RESAMPLE_FORMAT(DZN_SRC_F32);
    DZN_RESAMPLE_FORMAT(DZN_SRC_S16);
    DZN_RESAMPLE_FORMAT(DZN_SRC_U8);
    DZN_RESAMPLE_FORMAT(DZN_SRC_S24);
    DZN_RESAMPLE_FORMAT(DZN_SRC_S32);
    DZN_RESAMPLE_FORMAT(DZN_SRC_F32I);
    DZN_RESAMPLE_FORMAT(DZN_SRC_ULAW);
    DZN_RESAMPLE_FORMAT(DZN_SRC_ALAW);
  }
#undef DZN_RESAMPLE_FORMAT
#undef DZN_RESAMPLE_LAUNCH
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
