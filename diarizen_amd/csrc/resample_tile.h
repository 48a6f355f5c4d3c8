// resample_tile.h — the device code that resample.hip (one call, one recording) and ingest.hip (one launch, many descriptors)
// share: the stored-sample decode, the LDS slot rule, one tile of the polyphase resampler and one decoded frame.  Both kernels
// therefore make the same bits: the order of the float32 operations of an output sample depends on its index m alone.
//
// Include it AFTER DZN_CHECKED_TU(name): the DZN_CHECKs below count in the word of the translation unit that includes them.
#pragma once
#include "common.h"
#include "checked.h"

namespace {

constexpr int kResampleTile = 1024;      // output samples per workgroup (dzn_resample_tile)
constexpr int kThreads = 256;
constexpr size_t kMaxLds = 64 * 1024;

template <bool PAD>
__device__ __forceinline__ int lds_slot(int i) {
  return PAD ? i + (i >> 5) : i;
}

constexpr int kFormatBytes[DZN_SRC_FORMATS] = {4, 2, 1, 3, 4, 4, 1, 1};      // bytes per stored sample

// sample s (= frame * channels + channel; 64-bit: an hour of 48 kHz stereo is 3.5e8 samples, 24-bit: 1e9 bytes) of the stored
// frames as float32.  Every conversion is exact but the int32 one, which rounds to nearest even as numpy's astype does.
// The 24-bit form is read byte by byte (3-byte samples are not aligned); G.711 is the integer expansion of ITU-T G.711
// (audio.ulaw_table / alaw_table), not a table: 256 codes -> at most 13 / 12 magnitude bits, exact in float32.
template <int FMT>
__device__ __forceinline__ float stored_sample(const void* __restrict__ src, int64_t s) {
  if (FMT == DZN_SRC_S16) return (float)static_cast<const int16_t*>(src)[s] * (1.0f / 32768.0f);
  if (FMT == DZN_SRC_U8) return (float)((int)static_cast<const uint8_t*>(src)[s] - 128) * (1.0f / 128.0f);
  if (FMT == DZN_SRC_S24) {
    const uint8_t* b = static_cast<const uint8_t*>(src) + s * 3;
    const uint32_t u = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16);
    return (float)((int32_t)(u << 8) >> 8) * (1.0f / 8388608.0f);
  }
  if (FMT == DZN_SRC_S32) return (float)static_cast<const int32_t*>(src)[s] * (1.0f / 2147483648.0f);
  if (FMT == DZN_SRC_ULAW) {
    const int u = ~(int)static_cast<const uint8_t*>(src)[s] & 0xFF;
    const int t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7);
    return (float)((u & 0x80) ? 0x84 - t : t - 0x84) * (1.0f / 32768.0f);
  }
  if (FMT == DZN_SRC_ALAW) {
    const int a = (int)static_cast<const uint8_t*>(src)[s] ^ 0x55;
    const int e = (a >> 4) & 7, m = a & 0x0F;
    const int t = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (float)((a & 0x80) ? t : -t) * (1.0f / 32768.0f);
  }
  return static_cast<const float*>(src)[s];          // DZN_SRC_F32 / DZN_SRC_F32I
}

// tile `tile` of the range [m0, m1): output samples m0 + tile * kResampleTile .. (at most kResampleTile of them) -> dst[m - m0].
// The workgroup stages the input samples they read in xs (lds_floats floats of LDS), decoding the stored frames and
// zero-filling outside [0, T), then every lane walks the K taps of its output samples with ONE fp32 accumulator.
template <int FMT, bool PAD>
__device__ __forceinline__ void resample_tile(const void* __restrict__ src, int channels, int channel, int64_t src_first,
                                              int64_t src_len, int64_t T, const float* __restrict__ bank, int o, int n,
                                              int width, int K, int64_t m0, int64_t m1, float* __restrict__ dst, int tile,
                                              int lds_floats, float* __restrict__ xs) {
  const int tid = threadIdx.x;
  const int64_t mt0 = m0 + (int64_t)tile * kResampleTile;
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
        const int64_t s0 = r * channels;             // first sample of the frame
        DZN_CHECK(channel >= DZN_CHANNEL_DOWNMIX && channel < channels && (FMT != DZN_SRC_F32 || channels == 1), 0x824, channel);
        if (FMT == DZN_SRC_F32) {
          v = static_cast<const float*>(src)[r];
        } else if (channel >= 0) {                   // (wave-uniform)
          DZN_CHECK(s0 + channel < src_len * channels, 0x825, i);
          v = stored_sample<FMT>(src, s0 + channel);
        } else {                                     // downmix: running sum over the channels, one IEEE division
          DZN_CHECK(s0 + channels <= src_len * channels, 0x825, i);
          v = stored_sample<FMT>(src, s0);
          for (int c = 1; c < channels; ++c) v += stored_sample<FMT>(src, s0 + c);
          v /= (float)channels;
        }
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

// dst[r] = the channel choice of stored frame r of `frames` (the staging step above without the resampler)
template <int FMT>
__device__ __forceinline__ void decode_frame(const void* __restrict__ src, int channels, int channel, int64_t frames, int64_t r,
                                             float* __restrict__ dst) {
  const int64_t s0 = r * channels;                   // first sample of the frame
  DZN_CHECK(channel >= DZN_CHANNEL_DOWNMIX && channel < channels && (FMT != DZN_SRC_F32 || channels == 1), 0x826, channel);
  float v;
  if (FMT == DZN_SRC_F32) {
    v = static_cast<const float*>(src)[r];
  } else if (channel >= 0) {                         // (wave-uniform)
    DZN_CHECK(s0 + channel < frames * channels, 0x827, threadIdx.x);
    v = stored_sample<FMT>(src, s0 + channel);
  } else {                                           // downmix: running sum over the channels, one IEEE division
    DZN_CHECK(s0 + channels <= frames * channels, 0x827, threadIdx.x);
    v = stored_sample<FMT>(src, s0);
    for (int c = 1; c < channels; ++c) v += stored_sample<FMT>(src, s0 + c);
    v /= (float)channels;
  }
  dst[r] = v;
}

}  // namespace
