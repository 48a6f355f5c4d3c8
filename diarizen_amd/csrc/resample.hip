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

template <int FMT, bool PAD>
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

// dzn_decode: the staging loop of resample_kernel on its own, for a source that is already at the model's rate (the bank for
// equal rates is a low-pass, not the identity, so the resampler cannot serve it).  One stored frame per lane, consecutive
// lanes on consecutive frames; the downmix is the same running sum and ONE division.  No LDS, nothing tuned: a live chunk is
// a few KB and the call is launch-bound.
template <int FMT>
__global__ __launch_bounds__(kThreads) void decode_kernel(const void* __restrict__ src, int channels, int channel,
                                                          int64_t frames, float* __restrict__ dst) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= frames) return;
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
