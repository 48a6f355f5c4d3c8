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

#include "beamform_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

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
    gcc_phat_pair(R, Z, red_v, red_r, x + (int64_t)c * ch_stride, x_first, x_len, T, first, W, logW, max_lag, tw,
                  lag + (int64_t)c * nblk + blockIdx.x, peak + (int64_t)c * nblk + blockIdx.x);
  }
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
    DZN_CHECK(n - n0 >= 0 && n - n0 < n1 - n0, 0x85a, threadIdx.x);
    dst[n - n0] = beam_sample(x, channels, ch_stride, x_first, x_len, T, hop, logH, delay, num_blocks, n);
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
