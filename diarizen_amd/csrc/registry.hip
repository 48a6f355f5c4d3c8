// registry.hip — a device-resident, growing set of speaker identities and one sweep that matches a finished recording's
// voiceprints against it.
//
// No reference counterpart.  dzn_link_speakers (linkage.hip, §4.28) links a corpus that is complete: the n x n float64 matrix
// and the whole complete-linkage loop per call.  A registry keeps the voiceprints of everything linked so far on the device,
// each stored row under an identity number; a new recording needs only
//     D[k][i] = max over the stored rows r of identity i of cosdist(q_k, E_r)
// (the complete-linkage distance of query k to identity i), and of that table only the entries <= threshold: the caller's greedy
// assignment (diarizen_amd/registry.py) never looks at another.
//
//   storage   fp32 [capacity, dim] as given (NOT normalised: the distance is dzn_cdist_cosine's formula in float64), the row norms
//             float64 [capacity] (in-order sum, product and sum rounded separately, as row_norm_f32_kernel), both the registry's
//             own allocation.  The identity of every row lives on the host; the device holds the MEMBER INDEX built from it: the
//             rows sorted by identity (stable), cut into SEGMENTS — maximal runs of one identity inside a 64-entry chunk of the
//             sorted order — and per non-empty identity (a COLUMN) the range of its segments.  The index is rebuilt and uploaded
//             by the first match after an append.
//   registry_scan_kernel<NQ>   one wavefront per chunk of 64 index entries, one LANE PER STORED ROW.  The chunk's rows are fetched
//             in blocks of 32 floats: 8 lanes read 128 contiguous bytes of one row, the block is transposed through LDS
//             (stride 36 floats: ds_write_b128 / ds_read_b128 both conflict-free) so that every lane walks ITS row in order.
//             The queries of the group (NQ = 8, 16 or 32, the smallest that holds it) are float64 [dim][NQ] in global memory and
//             wave-uniform: they arrive by scalar loads and are the scalar operand of v_fma_f64, so the per-element cost is one
//             conversion and NQ fused multiply-adds for 64 rows, and the LDS carries each stored element once.  A float32 x
//             float32 product is exact in float64, so fma(x, q, acc) rounds exactly as the separate product and sum of the
//             definition do: one private in-order accumulator per (query, row).  cosine, clip, 1 - cosine per lane; then a
//             segmented max-scan over the lanes (keys: the segment ids, which ascend along the chunk) and the last lane of every
//             segment stores the segment's maxima with plain stores: no atomics, nothing to zero, and an identity of 10^4 members
//             is 157 independent segments.  Every stored byte is read once per group of up to 32 queries.
//   registry_reduce_kernel     one thread per (column, query): the max over the column's segments (independent loads) — the
//             table entry.  It is stored only when the dense table was asked for; an entry <= threshold is appended to the
//             (k, column, d) triples through one counter.  max is order-free, the host sorts the triples by (k, identity): the
//             output does not depend on the launch geometry or on arrival order.
// Uploads, scratch and launches use the host stage's device context (linkage.hip: its stream, arena and mutex), so a match may
// run in diarize_many's worker thread beside the engine.  Calls block; outputs are valid only after a clean drain.
#include <math.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "checked.h"
#include "common.h"

DZN_CHECKED_TU(registry)

namespace {

constexpr int R_CHUNK = 64;         // index entries per wavefront: one lane per stored row
constexpr int R_PASS = 8;           // staging passes per block: 8 lanes per row (128 contiguous bytes), 8 rows per pass
constexpr int R_DB = 32;            // floats of every row staged per block: 9 KB of LDS per wavefront
constexpr int R_LD = R_DB + 4;      // LDS row stride in floats: 36 = 4 (mod 32), b128 reads of 8 lanes cover the 32 banks
constexpr int R_QG = 32;            // queries per sweep at the most
constexpr int R_PUT_CHUNK = 8192;   // rows checked and uploaded at a time
// segment ids are int32 and there are at most capacity + capacity / 64 + 1 of them: the capacity ends where that would not fit
constexpr int64_t R_MAX_CAPACITY = (((int64_t)1 << 31) - 2 * R_CHUNK) / 65 * 64;
constexpr double R_DINF = __builtin_huge_val();

template <int NQ>
__global__ __launch_bounds__(R_CHUNK) void registry_scan_kernel(const float* __restrict__ vecs, const double* __restrict__ nrm,
                                                                const int* __restrict__ member, const int* __restrict__ segid,
                                                                int64_t n, int64_t rows, int dim, const double* __restrict__ qd,
                                                                int nq, double* __restrict__ partial, int64_t nseg, int qstride,
                                                                int qoff) {
  __shared__ __attribute__((aligned(16))) float tile[R_CHUNK * R_LD];
  __shared__ int srow[R_CHUNK];
  const int lane = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.x * R_CHUNK + lane;
  const bool valid = m < n;
  DZN_CHECK((int64_t)blockIdx.x * R_CHUNK < n, 0x8a0, blockIdx.x);
  const int row = member[valid ? m : n - 1];             // the overhang of the last chunk re-reads the last entry; masked below
  const int seg = valid ? segid[m] : -1;
  DZN_CHECK(row >= 0 && row < rows, 0x8a1, row);
  DZN_CHECK(!valid || (seg >= 0 && seg < nseg), 0x8a2, seg);
  srow[lane] = row;
  __syncthreads();
  double acc[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) acc[k] = 0.0;
  const int lr = lane >> 3, lc = 4 * (lane & 7);          // staging: 8 lanes per row, 8 rows per pass
  for (int d0 = 0; d0 < dim; d0 += R_DB) {
    const int dlen = dim - d0 < R_DB ? dim - d0 : R_DB;   // a multiple of 4
    const int gc = lc < dlen ? lc : dlen - 4;             // columns past the row's end re-read its last four: never used
    f32x4 g[R_PASS];
#pragma unroll
    for (int i = 0; i < R_PASS; ++i) {
      const int rr = R_PASS * i + lr;
      const int64_t o = (int64_t)srow[rr] * dim + d0 + gc;
      DZN_CHECK(rr < R_CHUNK && o >= 0 && o + 4 <= rows * dim, 0x8a3, rr);
      g[i] = *reinterpret_cast<const f32x4*>(vecs + o);
    }
    __syncthreads();                                      // the previous block has been read
#pragma unroll
    for (int i = 0; i < R_PASS; ++i) {
      const int w = (R_PASS * i + lr) * R_LD + lc;
      DZN_CHECK(w >= 0 && w + 4 <= R_CHUNK * R_LD, 0x8a4, w);
      *reinterpret_cast<f32x4*>(tile + w) = g[i];
    }
    __syncthreads();
    const double* qp = qd + (int64_t)d0 * NQ;
    for (int d4 = 0; d4 < dlen; d4 += 4) {
      DZN_CHECK(lane * R_LD + d4 + 4 <= R_CHUNK * R_LD, 0x8a4, d4);
      const f32x4 x = *reinterpret_cast<const f32x4*>(tile + lane * R_LD + d4);
      const double xd[4] = {(double)x[0], (double)x[1], (double)x[2], (double)x[3]};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NQ; ++k) acc[k] = fma(xd[j], qp[(d4 + j) * NQ + k], acc[k]);   // in order over dim; exact product
    }
  }
  // 1 - clip(dot / (|q| |e|)): dzn_cdist_cosine's expression
  const double* qn = qd + (int64_t)dim * NQ;
  const double ne = nrm[row];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const double den = qn[k] * ne;
    double cosine = acc[k] / den;
    if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);
    acc[k] = 1.0 - cosine;
  }
  // segmented max-scan: afterwards a lane holds the max over the lanes of its segment up to itself
#pragma unroll
  for (int o = 1; o < R_CHUNK; o <<= 1) {
    const int so = __shfl_up(seg, o, R_CHUNK);
    const bool take = lane >= o && so == seg;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const double v = __shfl_up(acc[k], o, R_CHUNK);
      acc[k] = fmax(acc[k], take ? v : acc[k]);
    }
  }
  const int sn = __shfl_down(seg, 1, R_CHUNK);
  if (valid && (lane == R_CHUNK - 1 || sn != seg)) {      // the last lane of its segment
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      if (k < nq) {
        const int64_t o = (int64_t)seg * qstride + qoff + k;
        DZN_CHECK(o >= 0 && o < nseg * qstride, 0x8a5, seg);
        partial[o] = acc[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void registry_reduce_kernel(const double* __restrict__ partial, const int* __restrict__ col_seg,
                                                              int64_t ncol, int Q, int64_t nseg, double threshold, int max_out,
                                                              double* __restrict__ dense, int* __restrict__ out_k,
                                                              int* __restrict__ out_c, double* __restrict__ out_d,
                                                              int* __restrict__ count) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ncol * Q) return;
  const int64_t c = idx / Q;
  const int q = (int)(idx - c * Q);
  const int s0 = col_seg[c], s1 = col_seg[c + 1];
  DZN_CHECK(s0 >= 0 && s0 < s1 && s1 <= nseg, 0x8a6, c);
  double v = -R_DINF;
  for (int s = s0; s < s1; ++s) v = fmax(v, partial[(int64_t)s * Q + q]);
  if (dense) {
    DZN_CHECK((int64_t)q * ncol + c < (int64_t)Q * ncol, 0x8a7, c);
    dense[(int64_t)q * ncol + c] = v;
  }
  if (v <= threshold) {
    const int pos = atomicAdd(count, 1);
    if (pos < max_out) {
      DZN_CHECK(pos >= 0, 0x8a8, pos);
      out_k[pos] = q;
      out_c[pos] = (int)c;
      out_d[pos] = v;
    }
  }
}

struct Registry {
  int device = -1, dim = 0;
  int64_t capacity = 0, rows = 0;
  float* vecs = nullptr;
  double* nrm = nullptr;
  int *member = nullptr, *segid = nullptr, *col_seg = nullptr;   // the member index: [capacity], [capacity], [capacity + 1]
  std::vector<int32_t> ident;         // per stored row
  std::vector<int32_t> col_ident;     // per column (non-empty identity, ascending): its identity number
  int64_t nseg = 0;
  int32_t max_ident = -1;
  bool index_dirty = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  mutable std::mutex mu;      // one append / match / rows / last_launch_ms of THIS registry at a time
};

#define RCHK(call)                                           \
  do {                                                       \
    if ((call) != hipSuccess) { rc = DZN_E_HIP; goto done; } \
  } while (0)

// |row| as row_norm_f32_kernel computes it; 0 = refuse the row (all zero or not finite)
double r_row_norm(const float* x, int dim) {
  double s = 0.0;
  for (int i = 0; i < dim; ++i) {
    if (!isfinite(x[i])) return 0.0;
    const double c = (double)x[i];
    const double p = c * c;
    s = s + p;
  }
  return sqrt(s);
}

// the member index from the identities: a stable counting sort, segments cut where the identity or the 64-entry chunk changes
void r_build_index(Registry* g, std::vector<int>& member, std::vector<int>& segid, std::vector<int>& col_seg) {
  const int64_t n = g->rows;
  // identity number -> column: a direct map while the numbers stay near the capacity, a search in the sorted numbers otherwise
  const bool direct = (int64_t)g->max_ident < 8 * g->capacity + 4096;
  std::vector<int32_t> ids;
  std::vector<int> col_of;
  if (direct) {
    col_of.assign((size_t)g->max_ident + 1, -1);
    for (int64_t r = 0; r < n; ++r) col_of[g->ident[r]] = 0;
    for (int64_t id = 0; id <= g->max_ident; ++id)
      if (col_of[id] == 0) { col_of[id] = (int)ids.size(); ids.push_back((int32_t)id); }
  } else {
    ids.assign(g->ident.begin(), g->ident.end());
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  }
  auto col = [&](int32_t id) { return direct ? col_of[id] : (int)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
  const int64_t ncol = (int64_t)ids.size();
  g->col_ident = ids;
  std::vector<int64_t> start((size_t)ncol + 1, 0);
  for (int64_t r = 0; r < n; ++r) ++start[col(g->ident[r]) + 1];
  for (int64_t c = 0; c < ncol; ++c) start[c + 1] += start[c];
  member.assign((size_t)n, 0);
  segid.assign((size_t)n, 0);
  col_seg.assign((size_t)ncol + 1, 0);
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t r = 0; r < n; ++r) member[fill[col(g->ident[r])]++] = (int)r;
  }
  int64_t seg = -1;
  for (int64_t c = 0; c < ncol; ++c) {
    col_seg[c] = (int)(seg + 1);
    for (int64_t p = start[c]; p < start[c + 1]; ++p) {
      if (p == start[c] || p % R_CHUNK == 0) ++seg;
      segid[p] = (int)seg;
    }
  }
  col_seg[ncol] = (int)(seg + 1);
  g->nseg = seg + 1;
}

template <int NQ>
void r_launch_scan(const Registry* g, const double* qd, int nq, double* partial, int qstride, int qoff, hipStream_t s) {
  const int64_t nchunk = (g->rows + R_CHUNK - 1) / R_CHUNK;
  hipLaunchKernelGGL(registry_scan_kernel<NQ>, dim3((unsigned)nchunk), dim3(R_CHUNK), 0, s, g->vecs, g->nrm, g->member, g->segid,
                     g->rows, g->rows, g->dim, qd, nq, partial, g->nseg, qstride, qoff);
}

int r_group_width(int nq) { return nq <= 8 ? 8 : nq <= 16 ? 16 : 32; }

}  // namespace

extern "C" int dzn_registry_create(int32_t device, int32_t dim, int64_t capacity, void** out) {
  if (!out) return DZN_E_INVALID;
  *out = nullptr;
  if (dim < 4 || dim > 1024 || dim % 4 != 0 || capacity < 1 || capacity > R_MAX_CAPACITY) return DZN_E_INVALID;
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  int rc = DZN_OK;
  Registry* g = new Registry();
  g->dim = dim;
  g->capacity = capacity;
  g->device = device;
  {
    HostScratch hs(device, 0);
    if (hs.rc != DZN_OK) { delete g; return hs.rc; }
    if (device < 0) RCHK(hipGetDevice(&g->device));
    if (hipMalloc(&g->vecs, (size_t)capacity * dim * sizeof(float)) != hipSuccess ||
        hipMalloc(&g->nrm, (size_t)capacity * sizeof(double)) != hipSuccess ||
        hipMalloc(&g->member, (size_t)capacity * sizeof(int)) != hipSuccess ||
        hipMalloc(&g->segid, (size_t)capacity * sizeof(int)) != hipSuccess ||
        hipMalloc(&g->col_seg, (size_t)(capacity + 1) * sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      rc = DZN_E_NOMEM;
      goto done;
    }
    RCHK(hipEventCreate(&g->ev0));
    RCHK(hipEventCreate(&g->ev1));
  }
done:
  if (rc != DZN_OK) {
    if (g->vecs) (void)hipFree(g->vecs);
    if (g->nrm) (void)hipFree(g->nrm);
    if (g->member) (void)hipFree(g->member);
    if (g->segid) (void)hipFree(g->segid);
    if (g->col_seg) (void)hipFree(g->col_seg);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    delete g;
    return rc;
  }
  *out = g;
  return DZN_OK;
}

extern "C" int dzn_registry_append(void* gp, const float* h_vecs, int64_t count, const int32_t* h_identity) {
  Registry* g = static_cast<Registry*>(gp);
  if (!g || count < 0) return DZN_E_INVALID;
  if (count == 0) return DZN_OK;
  if (!h_vecs || !h_identity) return DZN_E_INVALID;
  const int dim = g->dim;
  std::lock_guard<std::mutex> lk(g->mu);
  if (count > g->capacity - g->rows) return DZN_E_NOMEM;      // full: nothing written
  std::vector<double> nrm((size_t)count);
  int32_t top = g->max_ident;
  for (int64_t r = 0; r < count; ++r) {                        // everything is checked before anything is uploaded
    if (h_identity[r] < 0 || h_identity[r] == 0x7fffffff) return DZN_E_INVALID;
    nrm[r] = r_row_norm(h_vecs + r * dim, dim);
    if (!(nrm[r] > 0.0) || !isfinite(nrm[r])) return DZN_E_INVALID;
    if (h_identity[r] > top) top = h_identity[r];
  }
  int rc = DZN_OK;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  HostScratch hs(g->device, 0);
  if (hs.rc != DZN_OK) return hs.rc;
  for (int64_t r0 = 0; r0 < count; r0 += R_PUT_CHUNK) {
    const int64_t c = count - r0 < R_PUT_CHUNK ? count - r0 : R_PUT_CHUNK;
    RCHK(hipMemcpyAsync(g->vecs + (g->rows + r0) * dim, h_vecs + r0 * dim, (size_t)c * dim * sizeof(float),
                        hipMemcpyHostToDevice, hs.stream));
  }
  RCHK(hipMemcpyAsync(g->nrm + g->rows, nrm.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice, hs.stream));
done:
  if (hipStreamSynchronize(hs.stream) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;
  if (rc == DZN_OK) {      // the rows count only after a clean drain: a failed upload leaves the registry as it was
    g->ident.insert(g->ident.end(), h_identity, h_identity + count);
    g->rows += count;
    g->max_ident = top;
    g->index_dirty = true;
  }
  return rc;
}

extern "C" int dzn_registry_match(void* gp, const float* h_queries, int32_t Q, double threshold, int32_t max_out, int32_t* h_k,
                                  int32_t* h_i, double* h_d, int32_t* h_count, double* h_dense) {
  Registry* g = static_cast<Registry*>(gp);
  if (!g || !h_count || Q < 0 || max_out < 0 || !(threshold > 0.0 && threshold <= 2.0)) return DZN_E_INVALID;
  if (Q > 0 && !h_queries) return DZN_E_INVALID;
  if (max_out > 0 && (!h_k || !h_i || !h_d)) return DZN_E_INVALID;
  const int dim = g->dim;
  std::vector<double> qnorm((size_t)Q);
  for (int q = 0; q < Q; ++q) {
    qnorm[q] = r_row_norm(h_queries + (int64_t)q * dim, dim);
    if (!(qnorm[q] > 0.0) || !isfinite(qnorm[q])) return DZN_E_INVALID;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  const int64_t I = (int64_t)g->max_ident + 1;
  if (Q == 0 || g->rows == 0) {                                // nothing to compare: no launch
    *h_count = 0;
    return DZN_OK;
  }
  // the group images: per group float64 [dim][NQ] (query fastest), then the NQ norms; zero queries of norm 1 pad a group
  const int groups = (Q + R_QG - 1) / R_QG;
  std::vector<size_t> goff((size_t)groups + 1, 0);
  for (int gi = 0; gi < groups; ++gi) {
    const int nq = Q - gi * R_QG < R_QG ? Q - gi * R_QG : R_QG;
    goff[gi + 1] = goff[gi] + (size_t)(dim + 1) * r_group_width(nq);
  }
  std::vector<double> hq(goff[groups], 0.0);
  for (int gi = 0; gi < groups; ++gi) {
    const int nq = Q - gi * R_QG < R_QG ? Q - gi * R_QG : R_QG, NQ = r_group_width(nq);
    double* img = hq.data() + goff[gi];
    for (int k = 0; k < NQ; ++k) img[(size_t)dim * NQ + k] = 1.0;
    for (int k = 0; k < nq; ++k) {
      const float* src = h_queries + (int64_t)(gi * R_QG + k) * dim;
      for (int d = 0; d < dim; ++d) img[(size_t)d * NQ + k] = (double)src[d];
      img[(size_t)dim * NQ + k] = qnorm[gi * R_QG + k];
    }
  }
  int rc = DZN_OK;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  std::vector<int> member, segid, col_seg;
  if (g->index_dirty) r_build_index(g, member, segid, col_seg);
  const int64_t ncol = (int64_t)g->col_ident.size(), nseg = g->nseg;
  double *dq = nullptr, *partial = nullptr, *dense = nullptr, *out_d = nullptr;
  int *out_k = nullptr, *out_c = nullptr, *count = nullptr;
  auto carve = [&](char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
      char* p = base ? base + off : nullptr;
      off += (bytes + 255) & ~(size_t)255;
      return p;
    };
    dq = reinterpret_cast<double*>(take(hq.size() * sizeof(double)));
    partial = reinterpret_cast<double*>(take((size_t)nseg * Q * sizeof(double)));
    out_d = reinterpret_cast<double*>(take((size_t)max_out * sizeof(double) + 8));
    out_k = reinterpret_cast<int*>(take((size_t)max_out * sizeof(int) + 8));
    out_c = reinterpret_cast<int*>(take((size_t)max_out * sizeof(int) + 8));
    count = reinterpret_cast<int*>(take(sizeof(int)));
    if (h_dense) dense = reinterpret_cast<double*>(take((size_t)Q * ncol * sizeof(double)));
    return off;
  };
  HostScratch hs(g->device, carve(nullptr));
  if (hs.rc != DZN_OK) return hs.rc;
  carve(hs.base);
  hipStream_t s = hs.stream;
  int found = 0, got = 0;
  std::vector<int> hk, hc;
  std::vector<double> hd, hdense;
  if (g->index_dirty) {
    RCHK(hipMemcpyAsync(g->member, member.data(), member.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RCHK(hipMemcpyAsync(g->segid, segid.data(), segid.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RCHK(hipMemcpyAsync(g->col_seg, col_seg.data(), col_seg.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RCHK(hipStreamSynchronize(s));      // the index vectors are local
    g->index_dirty = false;
  }
  RCHK(hipMemcpyAsync(dq, hq.data(), hq.size() * sizeof(double), hipMemcpyHostToDevice, s));
  RCHK(hipMemsetAsync(count, 0, sizeof(int), s));
  RCHK(hipEventRecord(g->ev0, s));
  for (int gi = 0; gi < groups; ++gi) {
    const int nq = Q - gi * R_QG < R_QG ? Q - gi * R_QG : R_QG, NQ = r_group_width(nq);
    if (NQ == 8) r_launch_scan<8>(g, dq + goff[gi], nq, partial, Q, gi * R_QG, s);
    else if (NQ == 16) r_launch_scan<16>(g, dq + goff[gi], nq, partial, Q, gi * R_QG, s);
    else r_launch_scan<32>(g, dq + goff[gi], nq, partial, Q, gi * R_QG, s);
  }
  hipLaunchKernelGGL(registry_reduce_kernel, dim3((unsigned)((ncol * Q + 255) / 256)), dim3(256), 0, s, partial, g->col_seg, ncol,
                     Q, nseg, threshold, max_out, dense, out_k, out_c, out_d, count);
  RCHK(hipGetLastError());
  RCHK(hipEventRecord(g->ev1, s));
  g->timed = true;
  RCHK(hipMemcpyAsync(&found, count, sizeof(int), hipMemcpyDeviceToHost, s));
  RCHK(hipStreamSynchronize(s));
  got = found < max_out ? found : max_out;
  if (got > 0) {                                               // only the triples and their count cross the bus
    hk.resize(got); hc.resize(got); hd.resize(got);
    RCHK(hipMemcpyAsync(hk.data(), out_k, (size_t)got * sizeof(int), hipMemcpyDeviceToHost, s));
    RCHK(hipMemcpyAsync(hc.data(), out_c, (size_t)got * sizeof(int), hipMemcpyDeviceToHost, s));
    RCHK(hipMemcpyAsync(hd.data(), out_d, (size_t)got * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (h_dense) {
    hdense.resize((size_t)Q * ncol);
    RCHK(hipMemcpyAsync(hdense.data(), dense, hdense.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  }
done:
  if (hipStreamSynchronize(s) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;   // the outputs are only valid after a clean drain
  if (rc != DZN_OK) return rc;
  {
    std::vector<int> order((size_t)got);
    for (int j = 0; j < got; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return hk[a] != hk[b] ? hk[a] < hk[b] : hc[a] < hc[b]; });
    for (int j = 0; j < got; ++j) {
      h_k[j] = hk[order[j]];
      h_i[j] = g->col_ident[hc[order[j]]];
      h_d[j] = hd[order[j]];
    }
  }
  *h_count = found;
  if (h_dense) {                                               // [Q, I]: +inf where an identity number holds no stored row
    for (int64_t j = 0; j < (int64_t)Q * I; ++j) h_dense[j] = R_DINF;
    for (int q = 0; q < Q; ++q)
      for (int64_t c = 0; c < ncol; ++c) h_dense[(int64_t)q * I + g->col_ident[c]] = hdense[(size_t)q * ncol + c];
  }
  return DZN_OK;
}

extern "C" int dzn_registry_rows(const void* gp, int64_t* rows, int64_t* identities) {
  const Registry* g = static_cast<const Registry*>(gp);
  if (!g || !rows) return DZN_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  *rows = g->rows;
  if (identities) *identities = (int64_t)g->max_ident + 1;
  return DZN_OK;
}

extern "C" int dzn_registry_last_launch_ms(const void* gp, float* ms) {
  const Registry* g = static_cast<const Registry*>(gp);
  if (!g || !ms) return DZN_E_INVALID;
  std::lock_guard<std::mutex> lk(g->mu);
  if (!g->timed) return DZN_E_STATE;
  DeviceGuard dg(g->device);
  if (!dg.ok) return DZN_E_HIP;
  return hipEventElapsedTime(ms, g->ev0, g->ev1) == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_registry_destroy(void* gp) {
  Registry* g = static_cast<Registry*>(gp);
  if (!g) return DZN_OK;
  DeviceGuard dg(g->device);
  {
    std::lock_guard<std::mutex> lk(g->mu);      // a call in flight finishes first; the caller lets none begin after this
    HostScratch hs(g->device, 0);
    if (hs.rc == DZN_OK) (void)hipStreamSynchronize(hs.stream);
    (void)hipFree(g->vecs);
    (void)hipFree(g->nrm);
    (void)hipFree(g->member);
    (void)hipFree(g->segid);
    (void)hipFree(g->col_seg);
    (void)hipEventDestroy(g->ev0);
    (void)hipEventDestroy(g->ev1);
  }
  delete g;
  return DZN_OK;
}
