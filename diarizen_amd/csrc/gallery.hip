// gallery.hip — a device-resident gallery of enrolled voiceprints and one cosine search over it.
//
// No reference counterpart: the reference stops at anonymous cluster labels.  A voiceprint is a cluster centroid of the
// embeddings the engine already produces; identification scores a handful of such centroids (the queries) against every
// enrolled row and keeps the best top_n per query.  dzn_cdist_cosine (linkage.hip) uploads both operands per call, works in
// float64 with one thread per pair and returns the full matrix — right for 72 k x 13 once per recording, wrong for 16 queries
// against 10^6 resident rows on every hub tick, which is a 1 GB sweep that should run at the HBM rate and return 16 x n numbers.
//
//   storage   fp32 [capacity, dim], every row L2-normalised at put (norm in float64 with the in-order sum of
//             row_norm_f32_kernel, the quotient rounded ONCE to fp32), one validity byte per slot.  The rows are the gallery's
//             own allocation (not the host stage's arena: dzn_host_workspace_release leaves them alone).
//   gallery_scan_kernel   the group of up to 16 queries (one MFMA block) is the stationary operand, kept in LDS for the whole launch
//             in the order the MFMA wants it; workgroups stride over tiles of G_TILE rows, each wavefront streams one 16-row
//             MFMA tile straight from global memory into VGPRs with 16-byte loads (lane l: row l & 15, floats
//             16 s + 4 (l >> 4) .. + 3 of step s) and feeds v_mfma_f32_16x16x4_f32: element j of the load is k-slice l >> 4 of
//             the j-th MFMA of the step, and the query image holds the same k in the same place, so A and B agree on a
//             permuted k order.  fp32 inputs, fp32 accumulation: one fmaf chain of dim products per score.
//             Every gallery byte is read once per query group.  Selection: each workgroup keeps a sorted top-n per query in
//             LDS; a score is compared with the list's current n-th entry, the survivors are queued and inserted between two
//             barriers (one barrier when the tile queued nothing) by one wavefront per query, lane j holding list entry j: one
//             ballot finds the place, one store per lane moves the tail.  The lists go out as partials.
//   gallery_merge_kernel       per query, the partial lists (sorted) of all workgroups are merged by repeated selection of the
//             best list head: order (score descending, slot ascending), so duplicated rows tie and the lower slot wins.
//   dense     when asked for, the scan also stores every score — the same accumulator the selection saw, -inf at dropped
//             slots — which is what the tests check the selection against bit for bit.
// Uploads, scratch and launches use the host stage's device context (linkage.hip: its stream, arena and mutex), so a search
// may run in diarize_many's worker thread beside the engine.  Calls block; outputs are valid only after a clean drain.
#include <math.h>

#include <mutex>
#include <vector>

#include "checked.h"
#include "common.h"

DZN_CHECKED_TU(gallery)

namespace {

constexpr int G_TILE = 64;          // rows per workgroup tile: 4 wavefronts x one 16-row MFMA tile
constexpr int G_QG = 16;            // queries per group = one MFMA block.  Two blocks were measured: one sweep for 32 queries took
                                    // 0.73 ms at 2^20 x 256 against 2 x 0.28 ms for two sweeps of 16 (twice the LDS per workgroup
                                    // halves the workgroups per CU, and each inserts for twice the queries)
constexpr int G_TOPN = 32;          // list length in LDS = the largest top_n
constexpr int G_WG_PER_CU = 4;
constexpr int G_MAX_WG = 1024;      // the merge kernel gives every partial list a thread
constexpr int G_PUT_CHUNK = 8192;   // rows normalised and uploaded at a time

// (score descending, slot ascending); an empty entry is (-inf, INT_MAX) and loses to everything
__device__ __forceinline__ bool g_better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

constexpr size_t gallery_lds_bytes(int dim) {
  return (size_t)(dim / 16) * 64 * 16 + (size_t)G_QG * (G_TOPN * 8 + G_TILE * 8 + 4);
}

__global__ __launch_bounds__(256) void gallery_scan_kernel(const float* __restrict__ vecs, const uint8_t* __restrict__ valid,
                                                           int64_t rows, int dim, const float* __restrict__ queries, int nq,
                                                           int top_n, float* __restrict__ part_s, int* __restrict__ part_i,
                                                           float* __restrict__ dense) {
  extern __shared__ float4 g_smem[];
  constexpr int QG = G_QG;
  const int S = dim >> 4;                                   // 16-float steps per row
  float4* qs = g_smem;                                      // [S][64]: the lane's B fragment of every step
  float* ls = reinterpret_cast<float*>(qs + S * 64);        // [QG][G_TOPN] sorted scores
  int* li = reinterpret_cast<int*>(ls + QG * G_TOPN);       // [QG][G_TOPN] their slots (-1 = empty)
  float* qe_s = reinterpret_cast<float*>(li + QG * G_TOPN); // [QG][G_TILE] this tile's survivors
  int* qe_i = reinterpret_cast<int*>(qe_s + QG * G_TILE);
  int* qc = qe_i + QG * G_TILE;                             // [QG] survivors queued
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lr = lane & 15, kg = lane >> 4;
  const float NINF = -__builtin_huge_valf();

  for (int idx = t; idx < S * 64; idx += 256) {
    const int l = idx & 63, s = idx >> 6;
    qs[idx] = *reinterpret_cast<const float4*>(queries + (int64_t)(l & 15) * dim + 16 * s + 4 * (l >> 4));
  }
  for (int idx = t; idx < QG * G_TOPN; idx += 256) { ls[idx] = NINF; li[idx] = -1; }
  if (t < QG) qc[t] = 0;
  __syncthreads();

  const int64_t ntiles = (rows + G_TILE - 1) / G_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    DZN_CHECK(tile >= 0 && tile * G_TILE < rows, 0x840, tile);
    const int64_t row0 = tile * G_TILE + wave * 16;
    int64_t r = row0 + lr;
    r = r < rows ? r : rows - 1;                            // the overhang of the last tile re-reads the last row; masked below
    const float4* p = reinterpret_cast<const float4*>(vecs + r * dim) + kg;
    const int64_t srow = row0 + kg * 4;                     // the first of the 4 rows whose scores this lane receives
    uint8_t ok[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) ok[rr] = srow + rr < rows ? valid[srow + rr] : (uint8_t)0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < S; s0 += 16) {
      float4 g[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (s0 + i < S) g[i] = p[(s0 + i) * 4];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (s0 + i < S) {
          const float4 b = qs[(s0 + i) * 64 + lane];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].x, b.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].y, b.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].z, b.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(g[i].w, b.w, acc, 0, 0, 0);
        }
      }
    }
    // D: column (query) = lane & 15, row (of the 16-row tile) = 4 (lane >> 4) + register
    int queued = 0;
    const int q = lr;
    if (q < nq) {
      const float thr_s = ls[q * G_TOPN + top_n - 1];
      const int thr_i = li[q * G_TOPN + top_n - 1];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t slot = srow + rr;
        const float sc = ok[rr] ? acc[rr] : NINF;           // dropped or never-put slots, and the tile's overhang
        if (dense && slot < rows) dense[(int64_t)q * rows + slot] = sc;
        if (ok[rr] && g_better(sc, (int)slot, thr_s, thr_i < 0 ? 0x7fffffff : thr_i)) {
          const int pos = atomicAdd(&qc[q], 1);
          DZN_CHECK(pos >= 0 && pos < G_TILE, 0x842, pos);
          qe_s[q * G_TILE + pos] = sc;
          qe_i[q * G_TILE + pos] = (int)slot;
          queued = 1;
        }
      }
    }
    if (__syncthreads_or(queued)) {
      // every wavefront inserts for its share of the queries, lane j holding entry j of the sorted list: the entries that beat
      // the survivor are a prefix of length p, the others move one place down, the survivor lands at p
      for (int q = wave; q < QG; q += 4) {
        const int c = qc[q];
        const bool in = lane < top_n;
        for (int e = 0; e < c; ++e) {
          const float sc = qe_s[q * G_TILE + e];
          const int sl = qe_i[q * G_TILE + e];
          const float es = in ? ls[q * G_TOPN + lane] : NINF;
          const int ei = in ? li[q * G_TOPN + lane] : -1;
          const bool keep = in && g_better(es, ei < 0 ? 0x7fffffff : ei, sc, sl);
          const int p = __popcll(__ballot(keep));
          if (p < top_n) {                                  // (else an earlier insert moved the bar past it)
            if (in && lane >= p && lane + 1 < top_n) {
              ls[q * G_TOPN + lane + 1] = es;
              li[q * G_TOPN + lane + 1] = ei;
            }
            if (lane == p) {
              ls[q * G_TOPN + p] = sc;
              li[q * G_TOPN + p] = sl;
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next survivor reads what other lanes stored
        }
        if (lane == 0) qc[q] = 0;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int idx = t; idx < nq * top_n; idx += 256) {
    const int q = idx / top_n, j = idx - q * top_n;
    const int64_t o = ((int64_t)blockIdx.x * QG + q) * top_n + j;
    DZN_CHECK(o >= 0 && o < (int64_t)gridDim.x * QG * top_n, 0x841, o);
    part_s[o] = ls[q * G_TOPN + j];
    part_i[o] = li[q * G_TOPN + j];
  }
}

// one workgroup per query, one thread per partial list (nwg <= G_MAX_WG = blockDim): top_n rounds of "best head wins"
__global__ __launch_bounds__(G_MAX_WG) void gallery_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i,
                                                                 int nwg, int qg, int top_n, float* __restrict__ out_s,
                                                                 int64_t* __restrict__ out_i) {
  __shared__ float ws[G_MAX_WG / 64];
  __shared__ int wi[G_MAX_WG / 64];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float NINF = -__builtin_huge_valf();
  const int64_t base = ((int64_t)t * qg + q) * top_n;
  int head = 0;
  float hs = NINF;
  int hi = 0x7fffffff;
  auto fetch = [&]() {
    hs = NINF;
    hi = 0x7fffffff;
    if (t < nwg && head < top_n) {
      const int i = part_i[base + head];
      if (i >= 0) { hi = i; hs = part_s[base + head]; }
    }
  };
  fetch();
  for (int j = 0; j < top_n; ++j) {
    float bs = hs;
    int bi = hi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float s2 = __shfl_xor(bs, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (g_better(s2, i2, bs, bi)) { bs = s2; bi = i2; }
    }
    if (lane == 0) { ws[wave] = bs; wi[wave] = bi; }
    __syncthreads();
    bs = ws[0];
    bi = wi[0];
#pragma unroll
    for (int w = 1; w < G_MAX_WG / 64; ++w)
      if (g_better(ws[w], wi[w], bs, bi)) { bs = ws[w]; bi = wi[w]; }
    __syncthreads();
    const bool none = bi == 0x7fffffff;
    if (t == 0) {
      out_s[(int64_t)q * top_n + j] = none ? NINF : bs;
      out_i[(int64_t)q * top_n + j] = none ? (int64_t)-1 : (int64_t)bi;
    }
    if (!none && hi == bi) {      // slots are unique over the lists: exactly one thread owns the winner
      ++head;
      fetch();
    }
  }
}

struct Gallery {
  int device = -1, dim = 0, sweep_wg = 0;
  int64_t capacity = 0, rows = 0;      // rows = highest slot ever put + 1
  float* vecs = nullptr;
  uint8_t* valid = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;      // around a search's launches; evm: before the last merge
  bool timed = false;
  std::mutex mu;      // one put / drop / search of THIS gallery at a time (rows, the events)
};

#define GCHK(call)                                           \
  do {                                                       \
    if ((call) != hipSuccess) { rc = DZN_E_HIP; goto done; } \
  } while (0)

// |row| as row_norm_f32_kernel computes it: float64, in-order, product and sum rounded separately.  0 = refuse the row
// (all zero or not finite)
double g_row_norm(const float* x, int dim) {
  double s = 0.0;
  for (int i = 0; i < dim; ++i) {
    if (!isfinite(x[i])) return 0.0;
    const double c = (double)x[i];
    const double p = c * c;
    s = s + p;
  }
  return sqrt(s);
}

void g_normalise(const float* x, int dim, double nrm, float* out) {
  for (int i = 0; i < dim; ++i) out[i] = (float)((double)x[i] / nrm);
}

int g_launch_scan(const Gallery* g, int nwg, const float* dq, int nq, int top_n, float* part_s, int* part_i, float* dense,
                  hipStream_t s) {
  static unsigned long long mask = 0;
  if (first_use_on_device(mask) &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)gallery_lds_bytes(512)) != hipSuccess)
    return DZN_E_HIP;
  hipLaunchKernelGGL(gallery_scan_kernel, dim3(nwg), dim3(256), gallery_lds_bytes(g->dim), s, g->vecs, g->valid,
                     g->rows, g->dim, dq, nq, top_n, part_s, part_i, dense);
  return DZN_OK;
}

}  // namespace

extern "C" int dzn_gallery_create(int32_t device, int32_t dim, int64_t capacity, void** out) {
  if (!out) return DZN_E_INVALID;
  *out = nullptr;
  if (dim < 16 || dim > 512 || dim % 16 != 0 || capacity < 1 || capacity > ((int64_t)1 << 31) - 2 * G_TILE) return DZN_E_INVALID;
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  int rc = DZN_OK;
  Gallery* g = new Gallery();
  g->dim = dim;
  g->capacity = capacity;
  g->device = device;
  hipDeviceProp_t prop;
  {
    HostScratch hs(device, 0);
    if (hs.rc != DZN_OK) { delete g; return hs.rc; }
    if (device < 0) GCHK(hipGetDevice(&g->device));
    GCHK(hipGetDeviceProperties(&prop, g->device));
    g->sweep_wg = prop.multiProcessorCount * G_WG_PER_CU;
    if (g->sweep_wg > G_MAX_WG) g->sweep_wg = G_MAX_WG;
    if (g->sweep_wg < 1) g->sweep_wg = 1;
    if (hipMalloc(&g->vecs, (size_t)capacity * dim * sizeof(float)) != hipSuccess ||
        hipMalloc(&g->valid, (size_t)capacity) != hipSuccess) {
      (void)hipGetLastError();
      rc = DZN_E_NOMEM;
      goto done;
    }
    GCHK(hipEventCreate(&g->ev0));
    GCHK(hipEventCreate(&g->ev1));
    GCHK(hipEventCreate(&g->evm));
    GCHK(hipMemsetAsync(g->valid, 0, (size_t)capacity, hs.stream));
    GCHK(hipStreamSynchronize(hs.stream));
  }
done:
  if (rc != DZN_OK) {
    if (g->vecs) (void)hipFree(g->vecs);
    if (g->valid) (void)hipFree(g->valid);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->evm) (void)hipEventDestroy(g->evm);
    delete g;
    return rc;
  }
  *out = g;
  return DZN_OK;
}

extern "C" int dzn_gallery_put(void* gp, int64_t slot, const float* h_vecs, int64_t count) {
  Gallery* g = static_cast<Gallery*>(gp);
  if (!g || !h_vecs || slot < 0 || count < 1 || slot > g->capacity || count > g->capacity - slot) return DZN_E_INVALID;
  const int dim = g->dim;
  std::vector<double> nrm((size_t)count);
  for (int64_t r = 0; r < count; ++r) {
    nrm[r] = g_row_norm(h_vecs + r * dim, dim);
    if (!(nrm[r] > 0.0) || !isfinite(nrm[r])) return DZN_E_INVALID;      // before anything is uploaded
  }
  int rc = DZN_OK;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  std::lock_guard<std::mutex> lk(g->mu);
  HostScratch hs(g->device, 0);
  if (hs.rc != DZN_OK) return hs.rc;
  std::vector<float> stage((size_t)(count < G_PUT_CHUNK ? count : G_PUT_CHUNK) * dim);
  for (int64_t r0 = 0; r0 < count; r0 += G_PUT_CHUNK) {
    const int64_t n = count - r0 < G_PUT_CHUNK ? count - r0 : G_PUT_CHUNK;
    for (int64_t r = 0; r < n; ++r) g_normalise(h_vecs + (r0 + r) * dim, dim, nrm[r0 + r], stage.data() + r * dim);
    GCHK(hipMemcpyAsync(g->vecs + (slot + r0) * dim, stage.data(), (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice,
                        hs.stream));
    GCHK(hipStreamSynchronize(hs.stream));      // the staging block is reused
  }
  GCHK(hipMemsetAsync(g->valid + slot, 1, (size_t)count, hs.stream));
  if (slot + count > g->rows) g->rows = slot + count;
done:
  if (hipStreamSynchronize(hs.stream) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;
  return rc;
}

extern "C" int dzn_gallery_drop(void* gp, int64_t slot, int64_t count) {
  Gallery* g = static_cast<Gallery*>(gp);
  if (!g || slot < 0 || count < 1 || slot > g->capacity || count > g->capacity - slot) return DZN_E_INVALID;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  std::lock_guard<std::mutex> lk(g->mu);
  HostScratch hs(g->device, 0);
  if (hs.rc != DZN_OK) return hs.rc;
  if (hipMemsetAsync(g->valid + slot, 0, (size_t)count, hs.stream) != hipSuccess) return DZN_E_HIP;
  return hipStreamSynchronize(hs.stream) == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_gallery_search(void* gp, const float* h_queries, int32_t Q, int32_t top_n, float* h_scores,
                                  int64_t* h_slots, float* h_dense) {
  Gallery* g = static_cast<Gallery*>(gp);
  if (!g || !h_queries || !h_scores || !h_slots || Q < 1 || top_n < 1 || top_n > G_TOPN) return DZN_E_INVALID;
  const int dim = g->dim;
  const int groups = (Q + G_QG - 1) / G_QG;
  std::vector<float> hq((size_t)groups * G_QG * dim, 0.0f);        // zero rows pad the last group
  for (int q = 0; q < Q; ++q) {
    const double n = g_row_norm(h_queries + (int64_t)q * dim, dim);
    if (!(n > 0.0) || !isfinite(n)) return DZN_E_INVALID;
    g_normalise(h_queries + (int64_t)q * dim, dim, n, hq.data() + (size_t)q * dim);
  }
  std::lock_guard<std::mutex> lk(g->mu);
  const int64_t rows = g->rows;
  if (rows == 0) {                                                 // nothing was ever put: no launch
    for (int64_t i = 0; i < (int64_t)Q * top_n; ++i) { h_scores[i] = -__builtin_huge_valf(); h_slots[i] = -1; }
    return DZN_OK;
  }
  const int64_t ntiles = (rows + G_TILE - 1) / G_TILE;
  const int nwg = (int)(ntiles < g->sweep_wg ? ntiles : g->sweep_wg);
  int rc = DZN_OK;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  float *dq = nullptr, *part_s = nullptr, *out_s = nullptr, *dense = nullptr;
  int* part_i = nullptr;
  int64_t* out_i = nullptr;
  auto carve = [&](char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
      char* p = base ? base + off : nullptr;
      off += (bytes + 255) & ~(size_t)255;
      return p;
    };
    dq = reinterpret_cast<float*>(take(hq.size() * sizeof(float)));
    part_s = reinterpret_cast<float*>(take((size_t)nwg * G_QG * top_n * sizeof(float)));
    part_i = reinterpret_cast<int*>(take((size_t)nwg * G_QG * top_n * sizeof(int)));
    out_s = reinterpret_cast<float*>(take((size_t)Q * top_n * sizeof(float)));
    out_i = reinterpret_cast<int64_t*>(take((size_t)Q * top_n * sizeof(int64_t)));
    if (h_dense) dense = reinterpret_cast<float*>(take((size_t)Q * rows * sizeof(float)));
    return off;
  };
  HostScratch hs(g->device, carve(nullptr));
  if (hs.rc != DZN_OK) return hs.rc;
  carve(hs.base);
  hipStream_t s = hs.stream;
  GCHK(hipMemcpyAsync(dq, hq.data(), hq.size() * sizeof(float), hipMemcpyHostToDevice, s));
  GCHK(hipEventRecord(g->ev0, s));
  for (int gi = 0; gi < groups; ++gi) {
    const int nq = Q - gi * G_QG < G_QG ? Q - gi * G_QG : G_QG;
    const float* q0 = dq + (size_t)gi * G_QG * dim;
    float* d0 = dense ? dense + (size_t)gi * G_QG * rows : nullptr;
    rc = g_launch_scan(g, nwg, q0, nq, top_n, part_s, part_i, d0, s);
    if (rc != DZN_OK) goto done;
    if (gi == groups - 1) GCHK(hipEventRecord(g->evm, s));
    hipLaunchKernelGGL(gallery_merge_kernel, dim3(nq), dim3(G_MAX_WG), 0, s, part_s, part_i, nwg, G_QG, top_n,
                       out_s + (size_t)gi * G_QG * top_n, out_i + (size_t)gi * G_QG * top_n);
  }
  GCHK(hipGetLastError());
  GCHK(hipEventRecord(g->ev1, s));
  g->timed = true;
  GCHK(hipMemcpyAsync(h_scores, out_s, (size_t)Q * top_n * sizeof(float), hipMemcpyDeviceToHost, s));
  GCHK(hipMemcpyAsync(h_slots, out_i, (size_t)Q * top_n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (h_dense) GCHK(hipMemcpyAsync(h_dense, dense, (size_t)Q * rows * sizeof(float), hipMemcpyDeviceToHost, s));
done:
  if (hipStreamSynchronize(s) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;   // the outputs are only valid after a clean drain
  return rc;
}

extern "C" int dzn_gallery_geometry(const void* gp, int32_t* tile_rows, int32_t* sweep_rows, int32_t* query_group,
                                    int32_t* max_top_n) {
  const Gallery* g = static_cast<const Gallery*>(gp);
  if (!g || !tile_rows || !sweep_rows || !query_group || !max_top_n) return DZN_E_INVALID;
  *tile_rows = G_TILE;
  *sweep_rows = g->sweep_wg * G_TILE;
  *query_group = G_QG;
  *max_top_n = G_TOPN;
  return DZN_OK;
}

extern "C" int dzn_gallery_rows(const void* gp, int64_t* rows) {
  const Gallery* g = static_cast<const Gallery*>(gp);
  if (!g || !rows) return DZN_E_INVALID;
  *rows = g->rows;
  return DZN_OK;
}

extern "C" int dzn_gallery_last_launch_ms(const void* gp, float* ms, float* merge_ms) {
  const Gallery* g = static_cast<const Gallery*>(gp);
  if (!g || !ms) return DZN_E_INVALID;
  if (!g->timed) return DZN_E_STATE;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  if (merge_ms && hipEventElapsedTime(merge_ms, g->evm, g->ev1) != hipSuccess) return DZN_E_HIP;
  return hipEventElapsedTime(ms, g->ev0, g->ev1) == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_gallery_destroy(void* gp) {
  Gallery* g = static_cast<Gallery*>(gp);
  if (!g) return DZN_OK;
  DeviceGuard dg(g->device);
  {
    HostScratch hs(g->device, 0);
    if (hs.rc == DZN_OK) (void)hipStreamSynchronize(hs.stream);
    (void)hipFree(g->vecs);
    (void)hipFree(g->valid);
    (void)hipEventDestroy(g->ev0);
    (void)hipEventDestroy(g->ev1);
    (void)hipEventDestroy(g->evm);
  }
  delete g;
  return DZN_OK;
}
