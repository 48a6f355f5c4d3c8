// beamform_live.hip — array FEEDS on the device: what a live session adds to beamform.hip so that GCC-PHAT delay-and-sum runs in
// stream order without a host round trip (dzn_beamform_feed; DESIGN.md §4.24, include/dzn.h; the host forms are
// audio.causal_delays and testkit/beamform_live_ref.py).
//
// Kernel 1, decode_planar_kernel: the stored interleaved frames -> planar float32 [C][ch_stride] in ONE pass over the source.
// One frame per lane, consecutive lanes on consecutive frames; a lane walks the C samples of its frame (stored_sample of
// resample_tile.h: the conversions of dzn_decode, bit for bit), so the lines of the source are fetched once and each of the C
// stores of a wavefront is one coalesced row.  The offline path launches dzn_decode once per channel and reads the frames C
// times.  No LDS, nothing tuned: a live call holds a few blocks and is launch-bound.
//
// Kernel 2, track_kernel: the causal delay rule.  One lane per channel (C <= 64: one wavefront), sequential over the blocks
// [b0, b1).  Per channel the state is five int32: the held values of the four blocks before b0 (oldest first) and the number
// of blocks seen.  Block b: reliable = frame b holds >= hop samples of the recording and peak >= min_peak; held = reliable ?
// lag : the previous held value (0 before block 0); at block 0 the four history entries become held[0] (the left edge repeats
// the first entry); delay = the median of the history and held; the history shifts.  The result is a function of (state,
// columns) alone, so any partition of [0, nb) into consecutive calls gives one table and one final state.  Lags and the
// history are clamped to [-bound, bound] as they are read: |delay| <= bound whatever the buffers held, which is what lets the
// alignment pass read the table without a host check.  Plain vector loads and stores, no atomics, no LDS.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(beamform_live)

#include "resample_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

template <int FMT>
__global__ __launch_bounds__(kThreads) void decode_planar_kernel(const void* __restrict__ src, int channels, int64_t frames,
                                                                 float* __restrict__ dst, int64_t ch_stride) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= frames) return;
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

__global__ __launch_bounds__(DZN_WAVE) void track_kernel(const int* __restrict__ lag, const float* __restrict__ peak,
                                                         int64_t nblk, int channels, int ref, int hop, int64_t T, float min_peak,
                                                         int bound, int64_t b0, int64_t b1, int* __restrict__ state,
                                                         int* __restrict__ delay, int64_t delay_stride) {
  const int c = threadIdx.x;
  if (c >= channels) return;
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

int launch_decode_planar(const void* src, int format, int channels, int64_t frames, float* dst, int64_t ch_stride,
                         hipStream_t st) {
  if (frames < 0 || format < 0 || format >= DZN_SRC_FORMATS || channels < 1 || ch_stride < frames) return DZN_E_INVALID;
  if (frames == 0) return DZN_OK;
  const int64_t blocks = cdiv64(frames, kThreads);
  if (blocks > 0x7fffffff) return DZN_E_INVALID;
  ProfScope prof_scope_(st, "decode_planar", 0.0, (double)frames * channels * (kFormatBytes[format] + 4.0));
  const dim3 grid((unsigned)blocks), block(kThreads);
#define DZN_PLANAR_FORMAT(FMT)                                                                                  \
  case FMT:                                                                                                     \
    hipLaunchKernelGGL((decode_planar_kernel<FMT>), grid, block, 0, st, src, channels, frames, dst, ch_stride); \
    break
  switch (format) {
    DZN_PLANAR_FORMAT(DZN_SRC_F32);
    DZN_PLANAR_FORMAT(DZN_SRC_S16);
    DZN_PLANAR_FORMAT(DZN_SRC_U8);
    DZN_PLANAR_FORMAT(DZN_SRC_S24);
    DZN_PLANAR_FORMAT(DZN_SRC_S32);
    DZN_PLANAR_FORMAT(DZN_SRC_F32I);
    DZN_PLANAR_FORMAT(DZN_SRC_ULAW);
    DZN_PLANAR_FORMAT(DZN_SRC_ALAW);
  }
#undef DZN_PLANAR_FORMAT
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

int launch_beamform_track(const int* lag, const float* peak, int64_t nblk, int channels, int ref, int hop, int64_t T,
                          float min_peak, int bound, int64_t b0, int64_t b1, int* state, int* delay, int64_t delay_stride,
                          hipStream_t st) {
  if (b1 <= b0) return DZN_OK;
  if (channels < 1 || channels > DZN_WAVE || b1 - b0 > nblk || b1 > delay_stride) return DZN_E_INVALID;
  ProfScope prof_scope_(st, "beamform_track", 0.0, (double)(b1 - b0) * channels * 12.0);
  hipLaunchKernelGGL(track_kernel, dim3(1), dim3(DZN_WAVE), 0, st, lag, peak, nblk, channels, ref, hop, T, min_peak, bound, b0,
                     b1, state, delay, delay_stride);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
