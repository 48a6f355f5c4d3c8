// ingest.hip — the two kernels of a live hub's tick (diarizen_amd/hub.py) that take work from MANY sessions in one launch.
//
// dzn_ingest_many: a table of descriptors, each what one dzn_resample or dzn_decode call takes, and ONE launch.  One workgroup
// makes one tile of kResampleTile output samples (a decode descriptor: that many frames) of one descriptor; it finds the
// descriptor by a wave-uniform binary search over the tile prefix the host wrote (desc[d].tile0 = tiles owned by the
// descriptors before d; a descriptor without tiles shares its tile0 with its successor and is never found).  The descriptor's
// fields are then wave-uniform scalar loads, and format and LDS padding are wave-uniform run-time choices that dispatch to the
// SAME device code as the single-call kernels (resample_tile.h: resample_tile<FMT, PAD>, decode_frame<FMT>): one fp32
// accumulator over j = 0 .. K-1, the downmix a running sum and one division, so every output sample has the bits of the
// single call.  Dynamic LDS is the largest tile image of the table (at most 64 KiB).
//
// dzn_gather_windows: dst[b, :] = pool[offsets[b] : offsets[b] + window], the dense batch the engine's forward reads.  A row
// whose source and destination are both 16-byte aligned moves float4s (live offsets are multiples of the step); any other row
// takes the scalar path.  Both are streaming kernels: vector loads and stores, nothing else.
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(ingest)

#include "resample_tile.h"      // (after DZN_CHECKED_TU: its DZN_CHECKs count in this translation unit's word)

namespace {

template <int FMT>
__device__ __forceinline__ void ingest_tile(const dzn_ingest_desc* __restrict__ d, const uint8_t* __restrict__ stage,
                                            const float* __restrict__ banks, float* __restrict__ pool, int tile, int lds_floats,
                                            float* __restrict__ xs) {
  const void* src = stage + d->src_offset;
  float* dst = pool + d->dst_offset;
  const int channels = d->channels, channel = d->channel;
  const int64_t m0 = d->m0, m1 = d->m1;
  if (d->bank_offset < 0) {                          // decode-only: a feed at the model's rate (wave-uniform)
    const int64_t frames = m1 - m0;
    const int64_t r0 = (int64_t)tile * kResampleTile;
    const int64_t r1 = r0 + kResampleTile < frames ? r0 + kResampleTile : frames;
    DZN_CHECK(r0 < r1, 0x828, tile);
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kThreads) decode_frame<FMT>(src, channels, channel, frames, r, dst);
    return;
  }
  const int o = d->o, n = d->n, width = d->width, K = 2 * width + o;
  const float* bank = banks + d->bank_offset;
  if (o & 1)
    resample_tile<FMT, false>(src, channels, channel, d->src_first_index, d->src_len, d->total_len, bank, o, n, width, K, m0, m1,
                              dst, tile, lds_floats, xs);
  else                                               // even o: the padded LDS image
    resample_tile<FMT, true>(src, channels, channel, d->src_first_index, d->src_len, d->total_len, bank, o, n, width, K, m0, m1,
                             dst, tile, lds_floats, xs);
}

__global__ __launch_bounds__(kThreads) void ingest_many_kernel(const uint8_t* __restrict__ stage,
                                                               const dzn_ingest_desc* __restrict__ desc, int num_desc,
                                                               const float* __restrict__ banks, float* __restrict__ pool,
                                                               int lds_floats) {
  extern __shared__ float xs[];
  // the last descriptor whose tile0 <= this workgroup's tile (wave-uniform: blockIdx only)
  const int t = (int)blockIdx.x;
  int lo = 0, hi = num_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].tile0 <= t) lo = mid; else hi = mid - 1;
  }
  const dzn_ingest_desc* d = desc + lo;
  const int tile = t - d->tile0;
  DZN_CHECK(tile >= 0 && (int64_t)tile * kResampleTile < d->m1 - d->m0, 0x829, lo);
  if (tile < 0 || (int64_t)tile * kResampleTile >= d->m1 - d->m0) return;
  switch (d->src_format) {                           // (wave-uniform)
    case DZN_SRC_F32: ingest_tile<DZN_SRC_F32>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_S16: ingest_tile<DZN_SRC_S16>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_U8: ingest_tile<DZN_SRC_U8>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_S24: ingest_tile<DZN_SRC_S24>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_S32: ingest_tile<DZN_SRC_S32>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_F32I: ingest_tile<DZN_SRC_F32I>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_ULAW: ingest_tile<DZN_SRC_ULAW>(d, stage, banks, pool, tile, lds_floats, xs); break;
    case DZN_SRC_ALAW: ingest_tile<DZN_SRC_ALAW>(d, stage, banks, pool, tile, lds_floats, xs); break;
    default: DZN_CHECK(false, 0x82a, d->src_format); break;
  }
}

constexpr int kGatherVec = 4;            // floats per 16-byte access

__global__ __launch_bounds__(kThreads) void gather_windows_kernel(const float* __restrict__ pool,
                                                                  const int64_t* __restrict__ offsets, int B, int window,
                                                                  float* __restrict__ dst, int bases_aligned) {
  const int b = (int)blockIdx.y;
  DZN_CHECK(b < B, 0x82b, b);
  const int64_t off = offsets[b], out = (int64_t)b * window;      // (wave-uniform)
  const float* __restrict__ s = pool + off;
  float* __restrict__ y = dst + out;
  const int stride = (int)gridDim.x * kThreads;
  const int first = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  int done = 0;
  if (bases_aligned && !(off & (kGatherVec - 1)) && !(out & (kGatherVec - 1))) {
    const int nv = window / kGatherVec;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s);
    float4* __restrict__ y4 = reinterpret_cast<float4*>(y);
    for (int i = first; i < nv; i += stride) y4[i] = s4[i];
    done = nv * kGatherVec;
  }
  for (int i = done + first; i < window; i += stride) y[i] = s[i];
}

}  // namespace

int launch_ingest_many(const void* stage, const dzn_ingest_desc* desc, int num_desc, int64_t tiles, size_t lds_bytes,
                       double bytes_moved, const float* banks, float* pool, hipStream_t st) {
  if (num_desc < 0 || tiles < 0 || tiles > 0x7fffffff || lds_bytes > kMaxLds) return DZN_E_INVALID;
  if (num_desc == 0 || tiles == 0) return DZN_OK;
  ProfScope prof_scope_(st, "ingest_many", 0.0, bytes_moved);
  hipLaunchKernelGGL(ingest_many_kernel, dim3((unsigned)tiles), dim3(kThreads), lds_bytes, st,
                     static_cast<const uint8_t*>(stage), desc, num_desc, banks, pool, (int)(lds_bytes / sizeof(float)));
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

int launch_gather_windows(const float* pool, const int64_t* offsets, int B, int window, float* dst, hipStream_t st) {
  if (B < 0 || window < 1 || B > 65535) return DZN_E_INVALID;
  if (B == 0) return DZN_OK;
  ProfScope prof_scope_(st, "gather_windows", 0.0, 8.0 * (double)B * window);
  const int per_block = kThreads * kGatherVec;
  int gx = (window + per_block - 1) / per_block;
  gx = gx > 64 ? 64 : gx;                            // grid-stride beyond 64 workgroups per row
  const int aligned = !(reinterpret_cast<uintptr_t>(pool) & 15) && !(reinterpret_cast<uintptr_t>(dst) & 15);
  hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)gx, (unsigned)B), dim3(kThreads), 0, st, pool, offsets, B, window,
                     dst, aligned);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
