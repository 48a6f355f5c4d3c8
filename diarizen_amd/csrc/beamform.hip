// beamform.hip — array recordings on the device: GCC-PHAT time differences of arrival per (block, channel)
// (dzn_beamform_delays) and the delay-and-sum pass that aligns the channels and averages them into the one channel the engine
// diarizes (dzn_beamform_sum).  The algorithm is stated in DESIGN.md §4.23 and include/dzn.h; the host forms are
// audio.smooth_delays (between the two kernels) and testkit/beamform_ref.py (float64 / float32 numpy restatements).
//
// Kernel 1, gcc_phat_kernel: one workgroup per block b, W = 2 hop points.  Two complex float32 images live in LDS, 8 W bytes
// each (W = 8192: 2 x 64 KiB of the CU's 160 KiB, so one workgroup per CU): R, the spectrum of the reference channel, made
// once per block, and Z, which holds in turn the windowed frame of channel c, its spectrum, the PHAT-normalised cross spectrum
// and the correlation g.  The transforms are in-place radix-2: the forward one decimates in frequency (natural order in,
// bit-reversed order out), the product is pointwise, so both spectra may stay bit-reversed, and the inverse one decimates in
// time (bit-reversed in, natural out): no permutation pass.  Butterfly j of a stage with half-span m reads elements
// i0 = 2 (j - j % m) + j % m and i0 + m; lanes hold consecutive j.  For m >= 32 the 32 lanes of a ds_read_b64 group read 32
// consecutive float2 — one 256-byte bank row, no conflict.  For m < 32 (the five innermost stages of each transform) the group
// reads 32 of 64 consecutive float2: two bank rows, a 2-way conflict at the worst, which no padding of a LINEAR image improves
// (the lanes then meet one slot further on); the power-of-two strides that serialise an FFT in LDS arise when a LANE strides by
// m, which this lane assignment never does.  The twiddles (cos, -sin)(2 pi k / W), k < W / 2, come from the caller
// (audio.beamform_twiddle: float64, rounded once) and stay in L2 (32 KiB at W = 8192: with them in LDS two images no longer
// fit); the periodic Hann window is 0.5 -/+ 0.5 cos from the same table.  A transform is W / 2 log2 W butterflies of 10 flops:
// 0.53 Mflop at W = 8192, and 2 x 13 LDS round trips of 64 KiB.
//
// The real part of the inverse transform is g[l] W.  The argmax over l in [-L, L] follows the tie rule of the statement —
// visit 0, -1, +1, -2, +2, .. and keep a candidate only when strictly greater — as a reduction over (value, visiting rank)
// pairs: greater value wins, equal values go to the lower rank, which is associative and commutative, so the result does not
// depend on which lane saw what.  Nothing here depends on the launch: a block's lag and peak are functions of its frames.
//
// Kernel 2, delay_sum_kernel: one output sample per lane, consecutive lanes on consecutive n (coalesced reads of every channel,
// shifted by the block's delay), float32 running sum in ascending channel order, one IEEE division, and the cross-fade
// y = a + w (v - a) in three separately rounded operations (the build passes -ffp-contract=off; the intrinsics say so again).
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(beamform)

namespace {

constexpr int kGccThreadsMax = 1024;
constexpr int kSumThreads = 256;
constexpr int kSumTile = 1024;       // output samples per workgroup of delay_sum_kernel (dzn_beamform_tile)

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

__global__ __launch_bounds__(kGccThreadsMax) void gcc_phat_kernel(const float* __restrict__ x, int channels, int64_t ch_stride,
                                                                 int64_t x_first, int64_t x_len, int64_t T, int ref, int hop,
                                                                 int logW, int max_lag, const float2* __restrict__ tw,
                                                                 int64_t b0, int nblk, int* __restrict__ lag,
                                                                 float* __restrict__ peak) {
  extern __shared__ float2 lds[];
  __shared__ float red_v[kGccThreadsMax / DZN_WAVE];
  __shared__ int red_r[kGccThreadsMax / DZN_WAVE];
  const int W = hop << 1;
  float2* R = lds;
  float2* Z = lds + W;
  const int64_t b = b0 + blockIdx.x;
  const int64_t first = (b - 1) * (int64_t)hop;
  DZN_CHECK((int)blockIdx.x < nblk, 0x854, blockIdx.x);

  stage_frame(R, x + (int64_t)ref * ch_stride, x_first, x_len, T, first, W, tw);
  fft_forward(R, W, tw);
  if (threadIdx.x == 0) {
    lag[(int64_t)ref * nblk + blockIdx.x] = 0;
    peak[(int64_t)ref * nblk + blockIdx.x] = 0.f;
  }

  for (int c = 0; c < channels; ++c) {
    if (c == ref) continue;
    stage_frame(Z, x + (int64_t)c * ch_stride, x_first, x_len, T, first, W, tw);
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
      lag[(int64_t)c * nblk + blockIdx.x] = (rk & 1) ? -((rk + 1) >> 1) : (rk >> 1);
      peak[(int64_t)c * nblk + blockIdx.x] = v * (1.0f / (float)W);      // a power of two: exact
    }
    __syncthreads();      // red_* and Z are rewritten by the next channel
  }
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

__global__ __launch_bounds__(kSumThreads) void delay_sum_kernel(const float* __restrict__ x, int channels, int64_t ch_stride,
                                                                int64_t x_first, int64_t x_len, int64_t T, int hop, int logH,
                                                                const int* __restrict__ delay, int64_t num_blocks, int64_t n0,
                                                                int64_t n1, float* __restrict__ dst) {
  const int64_t base = n0 + (int64_t)blockIdx.x * kSumTile;
#pragma unroll
  for (int k = 0; k < kSumTile / kSumThreads; ++k) {
    const int64_t n = base + k * kSumThreads + threadIdx.x;
    if (n >= n1) return;
    const int64_t b = n >> logH;
    const float w = (float)(n - (b << logH)) / (float)hop;      // exact: hop is a power of two
    const float a = aligned_mean(x, channels, ch_stride, x_first, x_len, T, delay, num_blocks, b, n);
    const float v = aligned_mean(x, channels, ch_stride, x_first, x_len, T, delay, num_blocks, b + 1, n);
    DZN_CHECK(n - n0 >= 0 && n - n0 < n1 - n0, 0x85a, threadIdx.x);
    dst[n - n0] = __fadd_rn(a, __fmul_rn(w, __fsub_rn(v, a)));
  }
}

int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

}  // namespace

extern "C" int32_t dzn_beamform_tile(void) { return kSumTile; }

int launch_beamform_delays(const float* x, int channels, int64_t ch_stride, int64_t x_first, int64_t x_len, int64_t T, int ref,
                           int hop, int max_lag, const float* twiddle, int64_t b0, int64_t b1, int* lag, float* peak,
                           hipStream_t st) {
  if (b1 <= b0) return DZN_OK;
  if (b1 - b0 > 0x7fffffff) return DZN_E_INVALID;
  const int W = 2 * hop;
  const size_t lds = 2 * (size_t)W * sizeof(float2);
  static unsigned long long attr_mask = 0;
  if (first_use_on_device(attr_mask))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gcc_phat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * 8192 * (int)sizeof(float2));
  const int threads = hop < kGccThreadsMax ? hop : kGccThreadsMax;      // W / 2 butterflies per stage
  const int logW = ilog2(W);
  const double ffts = (double)(b1 - b0) * (2.0 * channels - 1.0);
  ProfScope prof_scope_(st, "beamform_delays", ffts * 5.0 * W * logW, (double)(b1 - b0) * channels * (4.0 * hop + 8.0));
  hipLaunchKernelGGL(gcc_phat_kernel, dim3((unsigned)(b1 - b0)), dim3(threads), lds, st, x, channels, ch_stride, x_first, x_len,
                     T, ref, hop, logW, max_lag, reinterpret_cast<const float2*>(twiddle), b0, (int)(b1 - b0), lag, peak);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

int launch_beamform_sum(const float* x, int channels, int64_t ch_stride, int64_t x_first, int64_t x_len, int64_t T, int hop,
                        const int* delay, int64_t num_blocks, int64_t n0, int64_t n1, float* dst, hipStream_t st) {
  if (n1 <= n0) return DZN_OK;
  const int64_t blocks = cdiv64(n1 - n0, kSumTile);
  if (blocks > 0x7fffffff) return DZN_E_INVALID;
  ProfScope prof_scope_(st, "beamform_sum", 2.0 * (double)(n1 - n0) * channels, (double)(n1 - n0) * 4.0 * (channels + 1));
  hipLaunchKernelGGL(delay_sum_kernel, dim3((unsigned)blocks), dim3(kSumThreads), 0, st, x, channels, ch_stride, x_first, x_len,
                     T, hop, ilog2(hop), delay, num_blocks, n0, n1, dst);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
