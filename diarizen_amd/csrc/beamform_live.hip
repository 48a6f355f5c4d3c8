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

#include "beamform_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

template <int FMT>
__global__ __launch_bounds__(kThreads) void decode_planar_kernel(const void* __restrict__ src, int channels, int64_t frames,
                                                                 float* __restrict__ dst, int64_t ch_stride) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= frames) return;
  planar_frame<FMT>(src, channels, frames, r, dst, ch_stride);
}

__global__ __launch_bounds__(DZN_WAVE) void track_kernel(const int* __restrict__ lag, const float* __restrict__ peak,
                                                         int64_t nblk, int channels, int ref, int hop, int64_t T, float min_peak,
                                                         int bound, int64_t b0, int64_t b1, int* __restrict__ state,
                                                         int* __restrict__ delay, int64_t delay_stride) {
  const int c = threadIdx.x;
  if (c >= channels) return;
  track_channel(lag, peak, nblk, c, ref, hop, T, min_peak, bound, b0, b1, state, delay, delay_stride);
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
