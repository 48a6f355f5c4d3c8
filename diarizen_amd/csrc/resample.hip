// resample.hip — the polyphase sinc resampler of the ingest path on the device (dzn_resample; torchaudio's
// functional.resample as Audio.downmix_and_resample calls it, PA/core/io.py:214-218; the host form is audio.resample).
//
//   y[m] = sum_{j < K} bank[p][j] * x[f o + j - width],   m = f n + p,  K = 2 width + o,  x = 0 outside [0, T)
//
// One workgroup makes kResampleTile consecutive output samples.  It stages the input samples they read — ((tile - 1) / n + 1) o
// + K at most — in LDS, converting int16 frames (sample * 2^-15, exact) and zero-filling outside the recording, then every
// lane walks the K taps of its output sample with ONE fp32 accumulator: acc = fmaf(tap_j, x_j, acc) for j = 0 .. K-1.  That
// order depends on m alone, not on the tile, the lane or the requested range, so a range call gives the bits of the same
// slice of a whole-recording call.
//
// Lanes hold consecutive m.  The bank is tap-major ([K][n]), so the taps of a wavefront are one coalesced read (n > 1: p runs
// with the lane) or a wave-uniform scalar read (n == 1).  The LDS reads of a wavefront are o floats apart for every n lanes
// (n lanes share a frame and broadcast): conflict-free for odd o; for even o (32 kHz -> 16 kHz: o = 2) the image carries one
// pad word per 32, which spreads the lanes of a 32-lane group over all 32 banks again.  The bank itself is not staged
// (44.1 kHz: 160 x 475 floats = 304 KB): it stays in L2.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(resample)

namespace {

constexpr int kResampleTile = 1024;      // output samples per workgroup (dzn_resample_tile)
constexpr int kThreads = 256;
constexpr size_t kMaxLds = 64 * 1024;

template <bool PAD>
__device__ __forceinline__ int lds_slot(int i) {
  return PAD ? i + (i >> 5) : i;
}

template <bool I16, bool PAD>
__global__ __launch_bounds__(kThreads) void resample_kernel(const void* __restrict__ src, int channels, int channel,
                                                            int64_t src_first, int64_t src_len, int64_t T,
                                                            const float* __restrict__ bank, int o, int n, int width, int K,
                                                            int64_t m0, int64_t m1, float* __restrict__ dst, int lds_floats) {
  extern __shared__ float xs[];
  const int tid = threadIdx.x;
  const int64_t mt0 = m0 + (int64_t)blockIdx.x * kResampleTile;
  const int64_t mt1 = mt0 + kResampleTile < m1 ? mt0 + kResampleTile : m1;
  const int64_t f0 = mt0 / n, f1 = (mt1 - 1) / n;
  const int64_t x0 = f0 * o - width;                 // input index of xs[0]
  const int span = (int)(f1 - f0) * o + K;
  DZN_CHECK(mt0 < mt1 && lds_slot<PAD>(span - 1) < lds_floats, 0x820, span);
  for (int i = tid; i < span; i += kThreads) {
    const int64_t a = x0 + i, r = a - src_first;
    float v = 0.f;
    if (a >= 0 && a < T) {
      DZN_CHECK(r >= 0 && r < src_len, 0x821, i);
      if (r >= 0 && r < src_len) {
        if (I16) v = (float)static_cast<const int16_t*>(src)[r * channels + channel] * (1.0f / 32768.0f);
        else v = static_cast<const float*>(src)[r];
      }
    }
    xs[lds_slot<PAD>(i)] = v;
  }
  __syncthreads();
  for (int64_t m = mt0 + tid; m < mt1; m += kThreads) {
    const int64_t f = m / n;
    const int p = (int)(m - f * n);
    const int xo = (int)(f - f0) * o;
    DZN_CHECK(xo >= 0 && xo + K <= span, 0x822, xo);
    float acc = 0.f;
    if (n == 1) {                                    // wave-uniform taps
#pragma unroll 4
      for (int j = 0; j < K; ++j) acc = fmaf(bank[j], xs[lds_slot<PAD>(xo + j)], acc);
    } else {
      const float* kp = bank + p;
      DZN_CHECK(p >= 0 && p < n, 0x823, p);
#pragma unroll 4
      for (int j = 0; j < K; ++j) acc = fmaf(kp[(int64_t)j * n], xs[lds_slot<PAD>(xo + j)], acc);
    }
    dst[m - m0] = acc;
  }
}

}  // namespace

extern "C" int32_t dzn_resample_tile(void) { return kResampleTile; }

// the LDS image of the widest tile: 0 when it does not fit (the caller refuses the ratio)
size_t resample_lds_bytes(int o, int n, int width) {
  const int64_t span = ((int64_t)(kResampleTile - 1) / n + 1) * o + 2 * (int64_t)width + o;
  const int64_t floats = (o & 1) ? span : span + (span >> 5) + 1;
  const size_t bytes = (size_t)floats * sizeof(float);
  return bytes <= kMaxLds ? bytes : 0;
}

int launch_resample(const void* src, int i16, int channels, int channel, int64_t src_first, int64_t src_len, int64_t T,
                    const float* bank, int o, int n, int width, int64_t m0, int64_t m1, float* dst, hipStream_t st) {
  const size_t lds = resample_lds_bytes(o, n, width);
  if (!lds || m1 < m0) return DZN_E_INVALID;
  if (m1 == m0) return DZN_OK;
  const int K = 2 * width + o;
  const int64_t blocks = cdiv64(m1 - m0, kResampleTile);
  if (blocks > 0x7fffffff) return DZN_E_INVALID;
  const double in_samples = (double)(m1 - m0) * o / n;
  ProfScope prof_scope_(st, "resample", 2.0 * (double)(m1 - m0) * K,
                        in_samples * (i16 ? 2.0 * channels : 4.0) + 4.0 * (double)(m1 - m0));
  const dim3 grid((unsigned)blocks), block(kThreads);
  const int lds_floats = (int)(lds / sizeof(float));
#define DZN_RESAMPLE_LAUNCH(I16, PAD)                                                                                  \
  hipLaunchKernelGGL((resample_kernel<I16, PAD>), grid, block, lds, st, src, channels, channel, src_first, src_len, T, \
                     bank, o, n, width, K, m0, m1, dst, lds_floats)
  const bool pad = !(o & 1);
  if (i16) { if (pad) DZN_RESAMPLE_LAUNCH(true, true); else DZN_RESAMPLE_LAUNCH(true, false); }
  else { if (pad) DZN_RESAMPLE_LAUNCH(false, true); else DZN_RESAMPLE_LAUNCH(false, false); }
#undef DZN_RESAMPLE_LAUNCH
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
