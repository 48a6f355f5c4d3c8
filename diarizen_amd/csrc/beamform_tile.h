// beamform_tile.h — the device code that beamform.hip / beamform_live.hip (one call, one recording) and beamform_many.hip (one
// launch set, many descriptors) share: the windowed frame, the two in-place radix-2 transforms, the GCC-PHAT body of one
// (block, channel) pair with its argmax, the aligned mean and the cross-faded output sample, one planar-decoded frame and the
// causal delay tracker.  Both sides therefore make the same bits: a block's lag and peak are functions of its frames, an output
// sample of its index, the table and the channels, and a tracked column of (state, columns) — never of the launch.  The
// algorithm and the LDS layout are stated at the top of beamform.hip and beamform_live.hip.
//
// Include it AFTER DZN_CHECKED_TU(name): the DZN_CHECKs below count in the word of the translation unit that includes them.
#pragma once
#include "common.h"
#include "checked.h"
#include "resample_tile.h"      // stored_sample<FMT>, kThreads

namespace {

constexpr int kGccThreadsMax = 1024;
constexpr int kGccHopMax = 4096;
constexpr int kSumThreads = 256;
constexpr int kSumTile = 1024;       // output samples per workgroup of the alignment pass (dzn_beamform_tile)

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// z[i] = hann[i] * x_c[(b - 1) hop + i], zero outside the recording
__device__ __forceinline__ void stage_frame(float2* z, const float* __restrict__ xc, int64_t x_first, int64_t x_len, int64_t T,
                                            int64_t first, int W, const float2* __restrict__ tw) {
  const int half = W >> 1;
  for (int i = threadIdx.x; i < W; i += blockDim.x) {
    const int64_t s = first + i;
    float v = 0.f;
    if (s >= 0 && s < T) {
      const int64_t at = s - x_first;
      DZN_CHECK(at >= 0 && at < x_len, 0x850, i);
      v = xc[at];
    }
    const float c = tw[i & (half - 1)].x;
    const float w = i < half ? 0.5f - 0.5f * c : 0.5f + 0.5f * c;
    z[i] = make_float2(v * w, 0.f);
  }
  __syncthreads();
}

// natural order in, bit-reversed order out
__device__ __forceinline__ void fft_forward(float2* z, int W, const float2* __restrict__ tw) {
  const int half = W >> 1;
  for (int m = half, sh = 0; m >= 1; m >>= 1, ++sh) {
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
      const int p = j & (m - 1);
      const int i0 = ((j - p) << 1) + p, i1 = i0 + m;
      DZN_CHECK(i1 < W && (p << sh) < half, 0x852, j);
      const float2 a = z[i0], c = z[i1];
      z[i0] = make_float2(a.x + c.x, a.y + c.y);
      z[i1] = cmul(make_float2(a.x - c.x, a.y - c.y), tw[p << sh]);
    }
    __syncthreads();
  }
}

// bit-reversed order in, natural order out, not scaled
__device__ __forceinline__ void fft_inverse(float2* z, int W, int logW, const float2* __restrict__ tw) {
  const int half = W >> 1;
  for (int m = 1, sh = logW - 1; m <= half; m <<= 1, --sh) {
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
      const int p = j & (m - 1);
      const int i0 = ((j - p) << 1) + p, i1 = i0 + m;
      DZN_CHECK(i1 < W && sh >= 0 && (p << sh) < half, 0x853, j);
      const float2 w = tw[p << sh];
      const float2 a = z[i0], t = cmul(z[i1], make_float2(w.x, -w.y));
      z[i0] = make_float2(a.x + t.x, a.y + t.y);
      z[i1] = make_float2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
}

// the better of two (value, visiting rank) candidates: strictly greater wins, equal values keep the earlier visit
__device__ __forceinline__ void keep_better(float& v, int& r, float v2, int r2) {
  if (v2 > v || (v2 == v && r2 < r)) { v = v2; r = r2; }
}

// One (block, channel) pair: R holds the bit-reversed spectrum of the reference frame, Z is scratch of W float2, red_v / red_r
// hold one entry per wavefront of the workgroup.  *lag_out / *peak_out are written by thread 0; the workgroup leaves through a
// barrier, so Z and red_* may be rewritten at once.
__device__ __forceinline__ void gcc_phat_pair(const float2* R, float2* Z, float* red_v, int* red_r,
                                              const float* __restrict__ xc, int64_t x_first, int64_t x_len, int64_t T,
                                              int64_t first, int W, int logW, int max_lag, const float2* __restrict__ tw,
                                              int* __restrict__ lag_out, float* __restrict__ peak_out) {
  stage_frame(Z, xc, x_first, x_len, T, first, W, tw);
  fft_forward(Z, W, tw);
  // G = X_c conj(X_ref) / |.|, 0 where the product is 0; scaled by its larger component first, so that neither the squares
  // of a faint bin underflow nor those of a loud one overflow
  for (int k = threadIdx.x; k < W; k += blockDim.x) {
    const float2 r = R[k], s = Z[k];
    float pr = s.x * r.x + s.y * r.y, pi = s.y * r.x - s.x * r.y;
    const float big = fmaxf(fabsf(pr), fabsf(pi));
    float2 g = make_float2(0.f, 0.f);
    if (big > 0.f && big <= 3.0e38f) {
      pr /= big;
      pi /= big;
      const float n = sqrtf(pr * pr + pi * pi);
      g = make_float2(pr / n, pi / n);
    }
    Z[k] = g;
  }
  __syncthreads();
  fft_inverse(Z, W, logW, tw);

  // argmax of Re Z[l mod W] over l in [-L, L]
  float v = Z[0].x;
  int rk = 0;
  for (int i = threadIdx.x; i < 2 * max_lag + 1; i += blockDim.x) {
    const int l = i - max_lag;
    const int at = (l + W) & (W - 1);
    DZN_CHECK(at >= 0 && at < W, 0x855, i);
    keep_better(v, rk, Z[at].x, l == 0 ? 0 : (l < 0 ? -2 * l - 1 : 2 * l));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int r2 = __shfl_xor(rk, o, 64);
    keep_better(v, rk, v2, r2);
  }
  const int wave = threadIdx.x / DZN_WAVE, waves = blockDim.x / DZN_WAVE;
  if ((threadIdx.x & (DZN_WAVE - 1)) == 0) {
    red_v[wave] = v;
    red_r[wave] = rk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < waves; ++w) keep_better(v, rk, red_v[w], red_r[w]);
    *lag_out = (rk & 1) ? -((rk + 1) >> 1) : (rk >> 1);
    *peak_out = v * (1.0f / (float)W);      // a power of two: exact
  }
  __syncthreads();      // red_* and Z are rewritten by the next pair
}

// S_b(n) = (sum_c x_c[n + delay[c, b]]) / C
__device__ __forceinline__ float aligned_mean(const float* __restrict__ x, int channels, int64_t ch_stride, int64_t x_first,
                                              int64_t x_len, int64_t T, const int* __restrict__ delay, int64_t num_blocks,
                                              int64_t b, int64_t n) {
  float s = 0.f;
  for (int c = 0; c < channels; ++c) {
    DZN_CHECK(b >= 0 && b < num_blocks, 0x858, c);
    const int64_t at = n + delay[(int64_t)c * num_blocks + b];
    float v = 0.f;
    if (at >= 0 && at < T) {
      DZN_CHECK(at - x_first >= 0 && at - x_first < x_len, 0x859, c);
      v = x[(int64_t)c * ch_stride + (at - x_first)];
    }
    s = c == 0 ? v : __fadd_rn(s, v);
  }
  return __fdiv_rn(s, (float)channels);
}

// y[n] = a + w (v - a) with a = S_b(n), v = S_{b+1}(n), w = (n - b hop) / hop: three separately rounded operations
__device__ __forceinline__ float beam_sample(const float* __restrict__ x, int channels, int64_t ch_stride, int64_t x_first,
                                             int64_t x_len, int64_t T, int hop, int logH, const int* __restrict__ delay,
                                             int64_t num_blocks, int64_t n) {
  const int64_t b = n >> logH;
  const float w = (float)(n - (b << logH)) / (float)hop;      // exact: hop is a power of two
  const float a = aligned_mean(x, channels, ch_stride, x_first, x_len, T, delay, num_blocks, b, n);
  const float v = aligned_mean(x, channels, ch_stride, x_first, x_len, T, delay, num_blocks, b + 1, n);
  return __fadd_rn(a, __fmul_rn(w, __fsub_rn(v, a)));
}

// stored frame r of `frames` -> dst[c * ch_stride + r] for every channel (the conversions of dzn_decode, bit for bit)
template <int FMT>
__device__ __forceinline__ void planar_frame(const void* __restrict__ src, int channels, int64_t frames, int64_t r,
                                             float* __restrict__ dst, int64_t ch_stride) {
  const int64_t s0 = r * channels;                   // first sample of the frame
  DZN_CHECK(r < ch_stride && s0 + channels <= frames * channels, 0x860, threadIdx.x);
  for (int c = 0; c < channels; ++c) dst[(int64_t)c * ch_stride + r] = stored_sample<FMT>(src, s0 + c);
}

__device__ __forceinline__ int clampi(int v, int bound) { return v < -bound ? -bound : (v > bound ? bound : v); }

__device__ __forceinline__ void order2(int& a, int& b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// the median of five (a sorting network cut down to the comparisons the middle element needs)
__device__ __forceinline__ int median5(int a, int b, int c, int d, int e) {
  order2(a, b);
  order2(d, e);
  order2(a, d);      // a is the least of a, b, d, e: not the median
  order2(b, e);      // e is the greatest of a, b, d, e: not the median
  order2(b, c);
  order2(c, d);
  order2(b, c);      // the median of b, c, d
  return c;
}

// the causal rule of channel c over blocks [b0, b1): compact lag / peak rows of stride nblk whose column 0 is block b0, the
// channel's five state ints, its row of the delay table.  Lags and state are clamped to [-bound, bound] as they are read.
__device__ __forceinline__ void track_channel(const int* __restrict__ lag, const float* __restrict__ peak, int64_t nblk, int c,
                                              int ref, int hop, int64_t T, float min_peak, int bound, int64_t b0, int64_t b1,
                                              int* __restrict__ state, int* __restrict__ delay, int64_t delay_stride) {
  int* s = state + c * DZN_BEAMFORM_STATE_INTS;
  int h0 = clampi(s[0], bound), h1 = clampi(s[1], bound), h2 = clampi(s[2], bound), h3 = clampi(s[3], bound);
  int seen = s[4];
  for (int64_t b = b0; b < b1; ++b) {
    DZN_CHECK(b - b0 < nblk && b < delay_stride, 0x862, c);
    const int64_t lo = (b - 1) * hop > 0 ? (b - 1) * hop : 0, hi = (b + 1) * hop < T ? (b + 1) * hop : T;
    const bool reliable = c != ref && hi - lo >= hop && peak[(int64_t)c * nblk + (b - b0)] >= min_peak;
    const int held = reliable ? clampi(lag[(int64_t)c * nblk + (b - b0)], bound) : (seen == 0 ? 0 : h3);
    if (seen == 0) h0 = h1 = h2 = h3 = held;
    delay[(int64_t)c * delay_stride + b] = c == ref ? 0 : median5(h0, h1, h2, h3, held);
    h0 = h1;
    h1 = h2;
    h2 = h3;
    h3 = held;
    ++seen;
  }
  s[0] = h0;
  s[1] = h1;
  s[2] = h2;
  s[3] = h3;
  s[4] = seen;
}

}  // namespace
