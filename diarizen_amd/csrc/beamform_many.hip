// beamform_many.hip — the beamforming of MANY array sessions in one fixed set of launches (dzn_beamform_many; a live hub's
// tick, diarizen_amd/hub.py).  A table of descriptors, each what one dzn_beamform_feed call takes, and four
// table-driven launches.  In every launch a workgroup finds its descriptor by a binary search over the prefix the host wrote
// for that launch (the ingest_many_kernel pattern: it reads blockIdx only, so the descriptor's fields are wave-uniform scalar
// loads; a descriptor without work shares its prefix with its successor and is never found); format and hop are wave-uniform
// run-time choices that dispatch to the SAME device code as the single-call kernels (beamform_tile.h), so every lag, peak,
// state, delay and output sample has the bits of dzn_beamform_feed.
//
// 1. decode_planar_many_kernel: one tile of kSumTile frames of one descriptor, a frame per lane and pass.
// 2. gcc_phat_many_kernel: one workgroup per (descriptor, block, non-reference channel).  gcc_phat_kernel runs one workgroup per
//    block and walks the C - 1 pairs in turn, which leaves a tick's handful of newly complete blocks on a handful of CUs; here
//    each pair has a workgroup of its own, which transforms the reference frame itself (identical inputs, identical bits) and
//    then its channel: 2 (C - 1) transforms per block instead of C + (C - 1), at most 1.5 times the flops, for C - 1 times the
//    workgroups.  Block size and dynamic LDS are those of the largest hop in the table; the loops of beamform_tile.h stride by
//    blockDim.x and the argmax is an associative, commutative reduction, so a smaller hop under more threads changes no bit
//    (surplus lanes hold the candidate of lag 0, which every lane starts from).
// 3. track_many_kernel: one wavefront per descriptor, a lane per channel, sequential over the descriptor's blocks.
// 4. delay_sum_many_kernel: one tile of kSumTile samples of [s_first, n1) of one descriptor; samples below n0 are copied from
//    the staging buffer of the call before (the history its resampler still reads), the others are delay-and-sum.
// Plain loads and stores throughout: no atomics, no inline assembly.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(beamform_many)

#include "beamform_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

// the last descriptor whose prefix field <= t (wave-uniform: t comes from blockIdx)
template <typename F>
__device__ __forceinline__ int find_desc(int num_desc, int t, F prefix) {
  int lo = 0, hi = num_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix(mid) <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int FMT>
__device__ __forceinline__ void decode_tile(const dzn_beamform_desc* __restrict__ d, const uint8_t* __restrict__ stage,
                                            float* __restrict__ planar, int tile) {
  const void* src = stage + d->src_offset;
  float* dst = planar + d->planar_offset;
  const int channels = d->channels;
  const int64_t frames = d->src_frames, ch_stride = d->ch_stride;
  const int64_t r0 = (int64_t)tile * kSumTile;
  const int64_t r1 = r0 + kSumTile < frames ? r0 + kSumTile : frames;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) planar_frame<FMT>(src, channels, frames, r, dst, ch_stride);
}

__global__ __launch_bounds__(kThreads) void decode_planar_many_kernel(const uint8_t* __restrict__ stage,
                                                                      const dzn_beamform_desc* __restrict__ desc, int num_desc,
                                                                      float* __restrict__ planar) {
  const int t = (int)blockIdx.x;
  const int at = find_desc(num_desc, t, [&](int i) { return desc[i].decode_tile0; });
  const dzn_beamform_desc* d = desc + at;
  const int tile = t - d->decode_tile0;
  DZN_CHECK(tile >= 0 && (int64_t)tile * kSumTile < d->src_frames, 0x870, at);
  if (tile < 0 || (int64_t)tile * kSumTile >= d->src_frames) return;
  switch (d->src_format) {                           // (wave-uniform)
    case DZN_SRC_F32: decode_tile<DZN_SRC_F32>(d, stage, planar, tile); break;
    case DZN_SRC_S16: decode_tile<DZN_SRC_S16>(d, stage, planar, tile); break;
    case DZN_SRC_U8: decode_tile<DZN_SRC_U8>(d, stage, planar, tile); break;
    case DZN_SRC_S24: decode_tile<DZN_SRC_S24>(d, stage, planar, tile); break;
    case DZN_SRC_S32: decode_tile<DZN_SRC_S32>(d, stage, planar, tile); break;
    case DZN_SRC_F32I: decode_tile<DZN_SRC_F32I>(d, stage, planar, tile); break;
    case DZN_SRC_ULAW: decode_tile<DZN_SRC_ULAW>(d, stage, planar, tile); break;
    case DZN_SRC_ALAW: decode_tile<DZN_SRC_ALAW>(d, stage, planar, tile); break;
    default: DZN_CHECK(false, 0x871, d->src_format); break;
  }
}

__global__ __launch_bounds__(kGccThreadsMax) void gcc_phat_many_kernel(const dzn_beamform_desc* __restrict__ desc, int num_desc,
                                                                      const float* __restrict__ twiddles,
                                                                      const float* __restrict__ planar, int* __restrict__ lag,
                                                                      float* __restrict__ peak, int lds_points) {
  extern __shared__ float2 lds[];
  __shared__ float red_v[kGccThreadsMax / DZN_WAVE];
  __shared__ int red_r[kGccThreadsMax / DZN_WAVE];
  const int t = (int)blockIdx.x;
  const int at = find_desc(num_desc, t, [&](int i) { return desc[i].gcc_item0; });
  const dzn_beamform_desc* d = desc + at;
  const int channels = d->channels, ref = d->ref, hop = d->hop;
  const int64_t nblk = d->b1 - d->b0;
  const int item = t - d->gcc_item0;
  const int blk = item / (channels - 1), k = item - blk * (channels - 1);
  DZN_CHECK(item >= 0 && blk < nblk && 4 * hop <= lds_points, 0x872, at);
  if (item < 0 || blk >= nblk || 4 * hop > lds_points) return;      // (wave-uniform)
  const int c = k < ref ? k : k + 1;                 // the k-th channel that is not the reference
  const int W = hop << 1;
  int logW = 0;
  while ((1 << logW) < W) ++logW;
  float2* R = lds;
  float2* Z = lds + W;
  const float2* tw = reinterpret_cast<const float2*>(twiddles + d->twiddle_offset);
  const float* x = planar + d->planar_offset;
  const int64_t ch_stride = d->ch_stride, x_first = d->src_first, x_len = d->src_frames, T = d->T;
  const int64_t first = (d->b0 + blk - 1) * (int64_t)hop;
  int* lg = lag + d->lag_offset;
  float* pk = peak + d->lag_offset;
  DZN_CHECK(c >= 0 && c < channels && c != ref && nblk <= d->blk_cap, 0x873, c);

  stage_frame(R, x + (int64_t)ref * ch_stride, x_first, x_len, T, first, W, tw);
  fft_forward(R, W, tw);
  if (k == 0 && threadIdx.x == 0) {                  // the lowest non-reference channel also writes the reference row
    lg[(int64_t)ref * nblk + blk] = 0;
    pk[(int64_t)ref * nblk + blk] = 0.f;
  }
  gcc_phat_pair(R, Z, red_v, red_r, x + (int64_t)c * ch_stride, x_first, x_len, T, first, W, logW, d->max_lag, tw,
                lg + (int64_t)c * nblk + blk, pk + (int64_t)c * nblk + blk);
}

__global__ __launch_bounds__(DZN_WAVE) void track_many_kernel(const dzn_beamform_desc* __restrict__ desc, int num_desc,
                                                              const int* __restrict__ lag, const float* __restrict__ peak,
                                                              int* __restrict__ state, int* __restrict__ delay) {
  const dzn_beamform_desc* d = desc + blockIdx.x;
  DZN_CHECK((int)blockIdx.x < num_desc, 0x874, blockIdx.x);
  const int c = threadIdx.x;
  if (c >= d->channels || d->b1 <= d->b0) return;
  track_channel(lag + d->lag_offset, peak + d->lag_offset, d->b1 - d->b0, c, d->ref, d->hop, d->T, d->min_peak, d->max_lag, d->b0,
                d->b1, state + d->state_offset, delay + d->delay_offset, d->table_blocks);
}

__global__ __launch_bounds__(kSumThreads) void delay_sum_many_kernel(const dzn_beamform_desc* __restrict__ desc, int num_desc,
                                                                     const float* __restrict__ planar,
                                                                     const int* __restrict__ delay, float* __restrict__ pool,
                                                                     float* __restrict__ beam) {
  const int t = (int)blockIdx.x;
  const int at = find_desc(num_desc, t, [&](int i) { return desc[i].sum_tile0; });
  const dzn_beamform_desc* d = desc + at;
  const int tile = t - d->sum_tile0;
  const int64_t s_first = d->s_first, n0 = d->n0, n1 = d->n1;
  DZN_CHECK(tile >= 0 && (int64_t)tile * kSumTile < n1 - s_first, 0x875, at);
  if (tile < 0 || (int64_t)tile * kSumTile >= n1 - s_first) return;
  const float* x = planar + d->planar_offset;
  const int* dl = delay + d->delay_offset;
  float* dst = (d->dst_space ? beam : pool) + d->dst_offset;
  const float* carry = beam + d->carry_offset;       // (read only below n0, where the call verified carry_offset >= 0)
  const int hop = d->hop;
  int logH = 0;
  while ((1 << logH) < hop) ++logH;
  const int64_t base = s_first + (int64_t)tile * kSumTile;
#pragma unroll
  for (int k = 0; k < kSumTile / kSumThreads; ++k) {
    const int64_t n = base + k * kSumThreads + threadIdx.x;
    if (n >= n1) return;
    DZN_CHECK(n >= s_first && (n >= n0 || d->carry_offset >= 0), 0x876, threadIdx.x);
    dst[n - s_first] = n < n0 ? carry[n - s_first]
                              : beam_sample(x, d->channels, d->ch_stride, d->src_first, d->src_frames, d->T, hop, logH, dl,
                                            d->table_blocks, n);
  }
}

}  // namespace

int launch_beamform_many(const void* stage, const dzn_beamform_desc* desc, int num_desc, int64_t decode_tiles, int64_t gcc_items,
                         int64_t sum_tiles, int max_hop, const double* work, const float* twiddles, float* planar,
                         int* lag, float* peak, int* state, int* delay, float* pool, float* beam, hipStream_t st) {
  if (num_desc < 0 || decode_tiles < 0 || gcc_items < 0 || sum_tiles < 0 || decode_tiles > 0x7fffffff || gcc_items > 0x7fffffff ||
      sum_tiles > 0x7fffffff || (gcc_items && (max_hop < 256 || max_hop > kGccHopMax)))
    return DZN_E_INVALID;
  if (num_desc == 0) return DZN_OK;
  if (decode_tiles) {
    ProfScope prof_scope_(st, "beamform_many_decode", 0.0, work[0]);
    hipLaunchKernelGGL(decode_planar_many_kernel, dim3((unsigned)decode_tiles), dim3(kThreads), 0, st,
                       static_cast<const uint8_t*>(stage), desc, num_desc, planar);
  }
  if (gcc_items) {
    static unsigned long long attr_mask = 0;
    if (first_use_on_device(attr_mask))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gcc_phat_many_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                4 * kGccHopMax * (int)sizeof(float2));
    const int threads = max_hop < kGccThreadsMax ? max_hop : kGccThreadsMax;
    {
      ProfScope prof_scope_(st, "beamform_many_delays", work[1], work[2]);
      hipLaunchKernelGGL(gcc_phat_many_kernel, dim3((unsigned)gcc_items), dim3(threads), 4 * (size_t)max_hop * sizeof(float2), st,
                         desc, num_desc, twiddles, planar, lag, peak, 4 * max_hop);
    }
    ProfScope prof_scope_(st, "beamform_many_track", 0.0, (double)gcc_items * 24.0);
    hipLaunchKernelGGL(track_many_kernel, dim3((unsigned)num_desc), dim3(DZN_WAVE), 0, st, desc, num_desc, lag, peak, state,
                       delay);
  }
  if (sum_tiles) {
    ProfScope prof_scope_(st, "beamform_many_sum", work[3], work[4]);
    hipLaunchKernelGGL(delay_sum_many_kernel, dim3((unsigned)sum_tiles), dim3(kSumThreads), 0, st, desc, num_desc, planar, delay,
                       pool, beam);
  }
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
