// linkage.hip — centroid-linkage agglomerative clustering with the distance matrix resident in HBM
// (row f1 of SURVEY.md §8f: host clustering scale-out), and the cosine distances of the assignment step.
//
// Replaces, for large inputs, the call
//     scipy.cluster.hierarchy.linkage(embeddings, method="centroid", metric="euclidean")
// of AgglomerativeClustering.cluster (PA/pipelines/clustering.py:407-416) and of the AHC
// initialisation of VBxClustering (PA/pipelines/clustering.py:656-658).  scipy forms the
// condensed n(n-1)/2 float64 distance matrix on the host and runs the generic O(n^2)..O(n^3)
// nearest-neighbour algorithm single-threaded: 17 s at 2 h of audio (36 k embeddings), minutes and
// 20 GB at 4 h — longer than the whole device stage on 8 GPUs.  Here:
//   * D [n][n] float64 lives in HBM (41 GB at n = 72 k; 288 GB available), filled by a tiled
//     pairwise-distance kernel (the diagonal holds +inf; retired columns keep their last distances and are
//     masked by size[], not blanked);
//   * the same greedy algorithm as scipy's fast_linkage runs on the device on LOWER BOUNDS: every row z keeps a
//     bound l1[z] of its minimum with a candidate neighbour n1[z] and a flag saying whether the bound is exact.  The
//     closest pair is the row with the smallest bound once that bound is exact; a stale bound is refreshed by
//     rescanning its row; a merge is the Lance-Williams centroid update of row / column `hi`, written in scipy's
//     operation order in float64;
//   * TWO remembered neighbours per row (l1 / n1, l2 / n2, flags): when a merge retires a row's nearest, the exact
//     second takes over without a rescan — 1.1-1.4 launches per merge (profiles/r6_linkage_top2.txt); the rules are
//     stated above step2_kernel and modelled in numpy in tests/test_design_math.py;
//   * ONE launch per step (step2_kernel): every workgroup of 256 rows reduces the same published per-workgroup
//     records to the same decision, then does its slice of the merge or of the rescan.  What a step publishes is
//     double-buffered by launch parity, so the kernel boundary is the only synchronisation;
//   * launches are queued in batches sized from the merges still missing (+ 1/8 + 32 for the expected rescans), the
//     step descriptor is read back between batches and surplus launches return at once: no host round trip inside
//     a batch.
// With no exact ties in the data the merge sequence — hence the dendrogram Z and every flat clustering cut from
// it — equals scipy's (tests/test_ops_gpu.py compares Z and fcluster output, also at edge sizes and with
// duplicated embeddings).
//
// The same loop under a second update rule links speakers ACROSS recordings (dzn_link_speakers): masked
// cosine distances (pdist_cosine_group_kernel: two rows of one recording are 4.0 apart), the complete-linkage update
// v = max(d_xi, d_yi) and a stop at the first closest pair above the threshold — step2_kernel<RULE_COMPLETE>.
//
// Retired forms: a two-kernel loop (single-workgroup selection + wide update per merge), the step loop with one
// remembered neighbour, and a single persistent launch whose workgroups exchanged records through polled slots.
// All three measured slower; their records are profiles/r3_linkage_step_vs_two_kernel.txt, profiles/r6_linkage_top2.txt
// and profiles/r6_linkage_persist.txt, and their source was last in the tree at commit 0d2d8c8.
#include <math.h>
#include <stdio.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "checked.h"
#include "common.h"

DZN_CHECKED_TU(linkage)

namespace {

constexpr double DINF = __builtin_huge_val();

// ---- pairwise euclidean distances, float64 accumulation: 64 x 64 tile per workgroup, j-tile >= i-tile ----
__global__ __launch_bounds__(256) void pdist_kernel(const float* __restrict__ E, int n, int dim,
                                                    double* __restrict__ D) {
  __shared__ float sa[64][17], sb[64][17];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // thread -> rows ty*4.., cols tx*4..
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < dim; k0 += 16) {
    for (int idx = threadIdx.x; idx < 64 * 16; idx += 256) {
      const int r = idx >> 4, c = idx & 15;
      const int gi = bi * 64 + r, gj = bj * 64 + r, gk = k0 + c;
      sa[r][c] = (gi < n && gk < dim) ? E[(int64_t)gi * dim + gk] : 0.f;
      sb[r][c] = (gj < n && gk < dim) ? E[(int64_t)gj * dim + gk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = (double)sa[ty * 4 + a][c];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = (double)sb[tx * 4 + b][c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = av[a] - bv[b];
          acc[a][b] += df * df;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = bi * 64 + ty * 4 + a, j = bj * 64 + tx * 4 + b;
      if (i < n && j < n) {
        const double d = i == j ? DINF : sqrt(acc[a][b]);
        D[(int64_t)i * n + j] = d;
        D[(int64_t)j * n + i] = d;
      }
    }
}

// row norms in float64, in-order sum (dzn_cdist_cosine and dzn_link_speakers)
__global__ __launch_bounds__(256) void row_norm_f32_kernel(const float* __restrict__ E, int n, int dim,
                                                           double* __restrict__ nrm) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float* e = E + (int64_t)r * dim;
  double s = 0.0;
  for (int i = 0; i < dim; ++i) {
    const double c = (double)e[i];
    const double p = c * c;
    s = s + p;
  }
  nrm[r] = sqrt(s);
}

// ---- pairwise cosine distances with a cannot-link mask (dzn_link_speakers): the tile and LDS staging of pdist_kernel ----
//     D[i][j] = group[i] == group[j] ? LINK_BIG : 1 - clip(dot(u_i, u_j) / (|u_i| |u_j|)),   D[i][i] = +inf
// scipy's pdist(E, "cosine") formula in float64: in-order sum over k, product and sum rounded separately (a float32 x float32
// product is exact in float64, so the sum is the same with or without contraction; it is switched off anyway).  LINK_BIG is
// FINITE on purpose: cosine distances end at 2, so 4 sorts above every real distance, and a finite value keeps the loop's
// "no finite distance left" test (STEP_FAIL) for NaN / inf input alone.  Complete linkage takes the max over member pairs,
// so a forbidden pair poisons every union that holds it: the mask is all the constraint needs.
constexpr double LINK_BIG = 4.0;

__global__ __launch_bounds__(256) void pdist_cosine_group_kernel(const float* __restrict__ E, const double* __restrict__ nrm,
                                                                 const int* __restrict__ group, int n, int dim,
                                                                 double* __restrict__ D) {
#pragma clang fp contract(off)
  __shared__ float sa[64][17], sb[64][17];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // thread -> rows ty*4.., cols tx*4..
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < dim; k0 += 16) {
    for (int idx = threadIdx.x; idx < 64 * 16; idx += 256) {
      const int r = idx >> 4, c = idx & 15;
      const int gi = bi * 64 + r, gj = bj * 64 + r, gk = k0 + c;
      DZN_CHECK(r < 64 && c < 16, 0x890, idx);
      DZN_CHECK(!(gi < n && gk < dim) || (int64_t)gi * dim + gk < (int64_t)n * dim, 0x891, gi);
      DZN_CHECK(!(gj < n && gk < dim) || (int64_t)gj * dim + gk < (int64_t)n * dim, 0x891, gj);
      sa[r][c] = (gi < n && gk < dim) ? E[(int64_t)gi * dim + gk] : 0.f;
      sb[r][c] = (gj < n && gk < dim) ? E[(int64_t)gj * dim + gk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = (double)sa[ty * 4 + a][c];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = (double)sb[tx * 4 + b][c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double p = av[a] * bv[b];
          acc[a][b] = acc[a][b] + p;
        }
    }
    __syncthreads();
  }
  double ni[4], nj[4];
  int gi[4], gj[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = bi * 64 + ty * 4 + a, j = bj * 64 + tx * 4 + a;
    DZN_CHECK(i >= 0 && j >= 0 && ty * 4 + a < 64 && tx * 4 + a < 64, 0x892, i);
    ni[a] = i < n ? nrm[i] : 1.0;
    gi[a] = i < n ? group[i] : 0;
    nj[a] = j < n ? nrm[j] : 1.0;
    gj[a] = j < n ? group[j] : 0;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = bi * 64 + ty * 4 + a, j = bj * 64 + tx * 4 + b;
      if (i < n && j < n) {
        const double den = ni[a] * nj[b];
        double cosine = acc[a][b] / den;
        if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);      // scipy clips the rounding error
        const double d = i == j ? DINF : gi[a] == gj[b] ? LINK_BIG : 1.0 - cosine;
        DZN_CHECK((int64_t)i * n + j < (int64_t)n * n && (int64_t)j * n + i < (int64_t)n * n, 0x893, i);
        D[(int64_t)i * n + j] = d;
        D[(int64_t)j * n + i] = d;
      }
    }
}

constexpr int SCAN_U = 8;   // loads in flight per thread in the row scan of init_rows2_kernel
constexpr int LB_BLK = 256;   // rows (= columns) per workgroup of the step loop

// block-wide minimum of per-thread (value, index) pairs, lowest index on ties; result valid in every thread
__device__ __forceinline__ void block_min_pair(double v, int id, double& val, int& idx, double* sval, int* sidx) {
  // wave reduction
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(id, o, 64);
    if (ov < v || (ov == v && oi < id)) { v = ov; id = oi; }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  __syncthreads();  // previous users of sval / sidx are done
  if (lane == 0) { sval[wave] = v; sidx[wave] = id; }
  __syncthreads();
  v = sval[0];
  id = sidx[0];
  for (int w = 1; w < nw; ++w) {
    const double ov = sval[w];
    const int oi = sidx[w];
    if (ov < v || (ov == v && oi < id)) { v = ov; id = oi; }
  }
  val = v;
  idx = id;
}

// ---- the step loop: ONE launch per step, TWO remembered neighbours per row ---------------------------------------------
// Every workgroup (256 rows / columns each) redundantly reduces the SAME published state — one record per workgroup: the
// minimum bound of its rows with that row's candidate neighbour and whether the bound is exact — so all of them reach the
// same decision without talking to each other, then each performs its slice of the step:
//   * MERGE  (bound exact): the Lance-Williams update of its columns, the two smallest of its slice of the new row, its
//     new record;
//   * RESCAN (bound stale): its slice of the row scan — spread over the chip — and its record with that row left out.
// What a step publishes (records, partial results, the step descriptor) is double-buffered by launch parity: a launch only
// READS what the previous launch wrote and only WRITES the other copy, so the kernel boundary is the only synchronisation.
// State with a single owner (bounds / neighbours / flags / size / cid of a row, the columns of D) is fixed up by the
// owner's thread at the start of the NEXT launch (the two neighbours of the merged or rescanned row from the partial
// results, the sizes of the merged pair); other workgroups substitute the previous step's values instead of reading those
// words.  Whether a bound is exact is tracked per row by the row's own thread instead of looked up in D.
//
// A launch is latency-bound (a chain of global round trips and block reductions on ~141 workgroups), so the kernel is written
// around the chain: (1) ONE round trip fetches everything that does not depend on the decision — the step descriptor, the
// published records and partial results, this thread's own row words; (2) one block reduction gives the fixed-up row's
// neighbours and the winner; (3) one round trip reads the two rows of D (or the slice of the rescanned row); (4) one block
// reduction publishes the partial result and the record.
//
// With one remembered neighbour 1.9-2.2 of every 3 launches were RESCANS: a merge retires the remembered neighbour of every
// row that pointed at `lo` or `hi`, those rows are the likeliest next winners, and each of them costs a whole launch before it
// can merge.  So every row keeps its TWO nearest neighbours:
//   I1: l1 <= D[z][c] for every active c != z;          e1: D[z][n1] == l1 (the exact minimum)
//   I2: l2 <= D[z][c] for every active c not in {z, n1}; e2: D[z][n2] == l2 (the exact second minimum, given e1)
// When a merge retires n1, the row's new minimum is min(new distance to the union, l2) and it is EXACT whenever e2 held (or the
// new distance undercuts the bound): the row merges without a rescan; the second slot then only keeps its bound (e2 = 0) until
// the next scan of the row refills both.  A numpy model of the rules is checked against scipy on the CPU
// (tests/test_design_math.py::test_linkage_top2_model_equals_scipy); on the 4 h recording's 20 888 embeddings the loop needs
// 1.1-1.3 launches per merge (profiles/r6_linkage_top2.txt).  The partial results of a row scan are top-2 pairs.
//
// The loop is indifferent to the update rule in every line but one: I1 / I2 / e1 / e2 are statements about bounds and hold for
// any new distance v of the union.  RULE picks that line at compile time:
//   RULE_CENTROID  scipy's Lance-Williams centroid update (dzn_linkage_centroid);
//   RULE_COMPLETE  v = max(d_xi, d_yi), and the loop STOPS at the first closest pair above `threshold` (dzn_link_speakers):
//                  the winner's bound is a lower bound of every distance left, so a bound above the threshold - exact or
//                  stale - means no merge at or below it remains.  The stop is STEP_DONE with k = the merges made.
enum { STEP_NONE = 0, STEP_MERGE = 1, STEP_RESCAN = 2, STEP_DONE = 3, STEP_FAIL = 4 };
enum { RULE_CENTROID = 0, RULE_COMPLETE = 1 };
struct StepState {
  int kind, lo, hi, nlo, nhi, k, x, pad;
  double dist;
};
struct StepRec {      // per workgroup: minimum bound of its rows
  double v;
  int x, y, exact, pad;
};
struct StepPart2 {    // per workgroup: the two smallest of its slice of a row (the merged row / the rescanned row)
  double v1, v2;
  int i1, i2;
};

__device__ __forceinline__ bool pair_lt(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }

// (v1, i1, v2, i2) <- the two smallest of {v1, v2, b1, b2} by (value, index); both inputs sorted, their elements distinct.
// Written as selects on values: the branchy form (assignments through references) was lowered to indexed SCRATCH stores -
// 64 B per lane of private memory and a memory round trip per merge, 10.8 us per launch where this form has 6.x.
__device__ __forceinline__ void top2_merge(double& v1, int& i1, double& v2, int& i2, double b1, int bi1, double b2, int bi2) {
  const double a1 = v1, a2 = v2;
  const int ai1 = i1, ai2 = i2;
  const bool bf = pair_lt(b1, bi1, a1, ai1);              // b's first is the overall first
  const double c1 = bf ? a1 : b1, c2 = bf ? b2 : a2;      // the two candidates for the second place
  const int ci1 = bf ? ai1 : bi1, ci2 = bf ? bi2 : ai2;
  const bool cs = pair_lt(c1, ci1, c2, ci2);
  v1 = bf ? b1 : a1;
  i1 = bf ? bi1 : ai1;
  v2 = cs ? c1 : c2;
  i2 = cs ? ci1 : ci2;
}

// Cross-lane moves of the wave reductions below as DPP controls (VALU data path, a few cycles) instead of `__shfl_xor`, which
// hipcc lowers to ds_bpermute_b32 (a round trip through the LDS crossbar per dword and stage: 108 of them chained in twelve
// dependent stages were ~1 us of every launch of a latency-bound kernel).  quad_perm [1,0,3,2] / [2,3,0,1], row_ror:4 / :8 give
// every lane of a 16-lane row the row's result (each stage joins DISJOINT lane sets, which top2_merge requires); row_bcast:15
// (into rows 1, 3) and row_bcast:31 (into rows 2, 3) carry it across rows - lanes outside the row mask receive `idle`, the
// identity of the reduction - and lane 63 ends up with the wave's result, read back with v_readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i(int idle, int v) {
  return __builtin_amdgcn_update_dpp(idle, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d(double idle, double v) {
  const int lo = dpp_i<CTRL, ROW_MASK>(__double2loint(idle), __double2loint(v));
  const int hi = dpp_i<CTRL, ROW_MASK>(__double2hiint(idle), __double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane63_d(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void top2_min_stage(double& a1, int& ai1, double& a2, int& ai2, double& m, int& mi) {
  const double b1 = dpp_d<CTRL, ROW_MASK>(DINF, a1), b2 = dpp_d<CTRL, ROW_MASK>(DINF, a2), bm = dpp_d<CTRL, ROW_MASK>(DINF, m);
  const int bi1 = dpp_i<CTRL, ROW_MASK>(0x7fffffff, ai1), bi2 = dpp_i<CTRL, ROW_MASK>(0x7fffffff, ai2),
            bmi = dpp_i<CTRL, ROW_MASK>(0x7fffffff, mi);
  top2_merge(a1, ai1, a2, ai2, b1, bi1, b2, bi2);
  if (pair_lt(bm, bmi, m, mi)) { m = bm; mi = bmi; }
}

// block-wide: the top-2 of per-thread sorted pairs (a1, ai1, a2, ai2) AND the minimum of per-thread (m, mi); valid in every
// thread.  sval: 12 doubles, sidx: 12 ints.
__device__ __forceinline__ void block_top2_min(double a1, int ai1, double a2, int ai2, double m, int mi, double& o1, int& oi1,
                                               double& o2, int& oi2, double& om, int& omi, double* sval, int* sidx) {
  top2_min_stage<0xB1, 0xf>(a1, ai1, a2, ai2, m, mi);      // quad_perm [1,0,3,2]
  top2_min_stage<0x4E, 0xf>(a1, ai1, a2, ai2, m, mi);      // quad_perm [2,3,0,1]
  top2_min_stage<0x124, 0xf>(a1, ai1, a2, ai2, m, mi);     // row_ror:4
  top2_min_stage<0x128, 0xf>(a1, ai1, a2, ai2, m, mi);     // row_ror:8
  top2_min_stage<0x142, 0xa>(a1, ai1, a2, ai2, m, mi);     // row_bcast:15 -> rows 1, 3
  top2_min_stage<0x143, 0xc>(a1, ai1, a2, ai2, m, mi);     // row_bcast:31 -> rows 2, 3
  a1 = readlane63_d(a1); a2 = readlane63_d(a2); m = readlane63_d(m);
  ai1 = __builtin_amdgcn_readlane(ai1, 63); ai2 = __builtin_amdgcn_readlane(ai2, 63); mi = __builtin_amdgcn_readlane(mi, 63);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;   // nw <= 4
  __syncthreads();
  if (lane == 0) {
    sval[wave] = a1; sval[4 + wave] = a2; sval[8 + wave] = m;
    sidx[wave] = ai1; sidx[4 + wave] = ai2; sidx[8 + wave] = mi;
  }
  __syncthreads();
  a1 = sval[0]; a2 = sval[4]; m = sval[8];
  ai1 = sidx[0]; ai2 = sidx[4]; mi = sidx[8];
  for (int w = 1; w < nw; ++w) {
    top2_merge(a1, ai1, a2, ai2, sval[w], sidx[w], sval[4 + w], sidx[4 + w]);
    if (pair_lt(sval[8 + w], sidx[8 + w], m, mi)) { m = sval[8 + w]; mi = sidx[8 + w]; }
  }
  o1 = a1; oi1 = ai1; o2 = a2; oi2 = ai2; om = m; omi = mi;
}

// initial state: the exact two nearest neighbours of every row (one workgroup per row) — the diagonal holds +inf
__global__ __launch_bounds__(256) void init_rows2_kernel(const double* __restrict__ D, int n, double* __restrict__ l1a,
                                                         double* __restrict__ l2a, int* __restrict__ n1a,
                                                         int* __restrict__ n2a, int* __restrict__ fla) {
  __shared__ double sval[12];
  __shared__ int sidx[12];
  const int z = blockIdx.x;
  const double* p = D + (int64_t)z * n;
  double v1 = DINF, v2 = DINF;
  int i1 = 0x7fffffff, i2 = 0x7fffffff;
  for (int i0 = threadIdx.x; i0 < n; i0 += SCAN_U * blockDim.x) {
    double xs[SCAN_U];
#pragma unroll
    for (int u = 0; u < SCAN_U; ++u) {
      const int i = i0 + u * blockDim.x;
      xs[u] = i < n ? p[i] : DINF;
    }
#pragma unroll
    for (int u = 0; u < SCAN_U; ++u) {
      const int i = i0 + u * blockDim.x;     // ascending per thread: strict comparisons keep the first occurrence
      if (xs[u] < v1) { v2 = v1; i2 = i1; v1 = xs[u]; i1 = i; }
      else if (xs[u] < v2) { v2 = xs[u]; i2 = i; }
    }
  }
  double o1, o2, om;
  int oi1, oi2, omi;
  block_top2_min(v1, i1, v2, i2, DINF, 0x7fffffff, o1, oi1, o2, oi2, om, omi, sval, sidx);
  if (threadIdx.x == 0) {
    const bool h1 = o1 < DINF, h2 = o2 < DINF;
    l1a[z] = o1; l2a[z] = o2; n1a[z] = h1 ? oi1 : -1; n2a[z] = h2 ? oi2 : -1; fla[z] = (h1 ? 1 : 0) | (h2 ? 2 : 0);
  }
}

__global__ __launch_bounds__(LB_BLK) void init_rec2_kernel(int n, const double* __restrict__ l1a, const int* __restrict__ n1a,
                                                           StepRec* __restrict__ rec) {
  __shared__ double sval[4];
  __shared__ int sidx[4];
  const int z = blockIdx.x * LB_BLK + threadIdx.x;
  double v;
  int x;
  block_min_pair(z < n ? l1a[z] : DINF, z < n ? z : 0x7fffffff, v, x, sval, sidx);
  if (z == x) {
    StepRec r;
    r.v = v; r.x = x; r.y = n1a[x]; r.exact = r.y >= 0; r.pad = 0;
    rec[blockIdx.x] = r;
  }
}

template <int RULE>
__global__ __launch_bounds__(LB_BLK) void step2_kernel(double* __restrict__ D, int n, double* __restrict__ l1a,
                                                       double* __restrict__ l2a, int* __restrict__ n1a, int* __restrict__ n2a,
                                                       int* __restrict__ fla, int* __restrict__ size, int* __restrict__ cid,
                                                       double* __restrict__ Z, StepState* __restrict__ st2,
                                                       StepRec* __restrict__ rec2, StepPart2* __restrict__ part2, int parity,
                                                       double threshold) {
  __shared__ double sval[12];
  __shared__ int sidx[12];
  __shared__ int sy[2];
  const int G = gridDim.x, w = blockIdx.x, t = threadIdx.x;
  const int z = w * LB_BLK + t;
  const bool in = z < n;
  const StepRec* rec = rec2 + (int64_t)parity * G;
  StepRec* rec_out = rec2 + (int64_t)(parity ^ 1) * G;
  const StepPart2* part = part2 + (int64_t)parity * G;
  StepPart2* part_out = part2 + (int64_t)(parity ^ 1) * G;
  StepState* st_out = st2 + (parity ^ 1);
  // ---- (1) everything that does not depend on the decision: ONE round trip ----
  const StepState prev = st2[parity];
  StepRec r0;
  r0.v = DINF; r0.x = 0x7fffffff; r0.y = -1; r0.exact = 0;
  StepPart2 p0;
  p0.v1 = p0.v2 = DINF; p0.i1 = p0.i2 = 0x7fffffff;
  if (t < G) { r0 = rec[t]; p0 = part[t]; }
  double my_l1 = in ? l1a[z] : DINF, my_l2 = in ? l2a[z] : DINF;
  int my_n1 = in ? n1a[z] : -1, my_n2 = in ? n2a[z] : -1, my_fl = in ? fla[z] : 0;
  int my_sz = in ? size[z] : 0;
  if (prev.kind == STEP_DONE || prev.kind == STEP_FAIL) {   // surplus launch: keep both copies of the descriptor final
    if (w == 0 && t == 0) *st_out = prev;
    return;
  }
  const bool owed = prev.kind == STEP_MERGE || prev.kind == STEP_RESCAN;
  // ---- (2) the two neighbours owed to the row of the previous step + the winner over the records ----
  double a1 = owed ? p0.v1 : DINF, a2 = owed ? p0.v2 : DINF, uv = r0.v;
  int ai1 = owed ? p0.i1 : 0x7fffffff, ai2 = owed ? p0.i2 : 0x7fffffff, ui = r0.x;
  for (int i = t + LB_BLK; i < G; i += LB_BLK) {            // n > 65 536 only
    const StepRec r = rec[i];
    const StepPart2 p = part[i];
    if (owed) top2_merge(a1, ai1, a2, ai2, p.v1, p.i1, p.v2, p.i2);
    if (pair_lt(r.v, r.x, uv, ui)) { uv = r.v; ui = r.x; }
  }
  double ev1, ev2, d;
  int eid1, eid2, x;
  block_top2_min(a1, ai1, a2, ai2, uv, ui, ev1, eid1, ev2, eid2, d, x, sval, sidx);
  const int ex = !owed ? 0x7fffffff : prev.kind == STEP_MERGE ? prev.hi : prev.x;   // the row left out of the records
  const int ey = ev1 < DINF ? eid1 : -1;
  bool dirty = false, sz_dirty = false;
  if (owed && z == ex) {
    my_l1 = ev1; my_n1 = ey; my_l2 = ev2; my_n2 = ev2 < DINF ? eid2 : -1;
    my_fl = (my_n1 >= 0 ? 1 : 0) | (my_n2 >= 0 ? 2 : 0);
    dirty = true;
  }
  if (prev.kind == STEP_MERGE) {
    if (z == prev.hi) { my_sz = prev.nlo + prev.nhi; cid[z] = n + prev.k - 1; sz_dirty = true; }
    if (z == prev.lo) { my_sz = 0; sz_dirty = true; }
  }
  const int k = prev.k;
  int y;
  bool exact;
  const bool extra_wins = owed && pair_lt(ev1, ex, d, x);
  if (extra_wins) {
    d = ev1; x = ex; y = ey; exact = ey >= 0;
  } else {
    __syncthreads();
    if (t < G && r0.x == x && r0.v == d) { sy[0] = r0.y; sy[1] = r0.exact; }
    for (int i = t + LB_BLK; i < G; i += LB_BLK)
      if (rec[i].x == x && rec[i].v == d) { sy[0] = rec[i].y; sy[1] = rec[i].exact; }
    __syncthreads();
    y = sy[0];
    exact = sy[1] != 0 && y >= 0;
  }
  if (!(d < DINF) || x < 0 || x >= n) {    // NaN / inf distances: no pair left to merge
    if (w == 0 && t == 0) { StepState s = prev; s.kind = STEP_FAIL; *st_out = s; }
    return;
  }
  if (RULE == RULE_COMPLETE && d > threshold) {   // every distance left is >= d: the merges at or below the threshold are made
    if (w == 0 && t == 0) { StepState s = prev; s.kind = STEP_DONE; *st_out = s; }
    return;
  }
  double pv = DINF;       // this thread's element of the row whose two smallest the step publishes
  int excl = -1;          // row left out of this step's records
  if (!exact) {
    // ---- RESCAN: this workgroup's slice of row x over the active columns (D[x][x] is +inf) ----
    if (w == 0 && t == 0) {
      StepState s = prev;
      s.kind = STEP_RESCAN; s.x = x; s.k = k; s.pad = prev.pad + 1;   // pad counts the rescans (diagnostics)
      *st_out = s;
    }
    if (in && my_sz != 0) pv = D[(int64_t)x * n + z];
    excl = x;
  } else {
    // ---- MERGE: Lance-Williams update of this workgroup's columns ----
    const int lo = x < y ? x : y, hi = x < y ? y : x;
    const bool sub = prev.kind == STEP_MERGE;    // words of the previous pair are being rewritten by their owners
    const int nlo = sub && lo == prev.hi ? prev.nlo + prev.nhi : size[lo];   // (lo / hi are active: never prev.lo)
    const int nhi = sub && hi == prev.hi ? prev.nlo + prev.nhi : size[hi];
    if (w == 0 && t == 0) {
      const int ia = sub && lo == prev.hi ? n + prev.k - 1 : cid[lo];
      const int ib = sub && hi == prev.hi ? n + prev.k - 1 : cid[hi];
      Z[4 * k + 0] = (double)(ia < ib ? ia : ib);
      Z[4 * k + 1] = (double)(ia < ib ? ib : ia);
      Z[4 * k + 2] = d;
      Z[4 * k + 3] = (double)(nlo + nhi);
      StepState s;
      s.kind = k + 1 >= n - 1 ? STEP_DONE : STEP_MERGE;
      s.lo = lo; s.hi = hi; s.nlo = nlo; s.nhi = nhi; s.k = k + 1; s.x = -1; s.pad = prev.pad; s.dist = d;
      *st_out = s;
    }
    if (in) {
      if (z == hi) {
        D[(int64_t)hi * n + lo] = DINF;
        my_l1 = my_l2 = DINF; my_n1 = my_n2 = -1; my_fl = 0; dirty = true;   // both neighbours at the start of the next launch
      } else if (z == lo) {
        my_l1 = my_l2 = DINF; my_fl = 0; dirty = true;                       // retired
      } else if (my_sz != 0) {
        const double dxi = D[(int64_t)lo * n + z], dyi = D[(int64_t)hi * n + z];
        // scipy _hierarchy_distance_update.pxi, _centroid(d_xi, d_yi, d_xy, size_x, size_y, size_i), same order; _complete
        const double v = RULE == RULE_COMPLETE
                             ? fmax(dxi, dyi)
                             : sqrt((((nlo * dxi * dxi) + (nhi * dyi * dyi)) - (nlo * nhi * d * d) / (nlo + nhi)) / (nlo + nhi));
        D[(int64_t)hi * n + z] = v;
        D[(int64_t)z * n + hi] = v;              // column lo is NOT blanked: readers of a row mask by size[]
        pv = v;
        // columns lo and (old) hi leave the row, column hi re-enters with v: the rules of the header (I1 / I2 / e1 / e2)
        const bool d1 = my_n1 == lo || my_n1 == hi, d2 = my_n2 == lo || my_n2 == hi;
        const bool e1 = my_fl & 1, e2 = my_fl & 2;
        if (!d1) {
          if (v < my_l1) {                       // the union is the new nearest: exact whatever l1 was
            my_l2 = my_l1; my_n2 = my_n1; my_fl = 1 | (e1 ? 2 : 0);
            my_l1 = v; my_n1 = hi; dirty = true;
          } else if (!d2) {
            if (v < my_l2) { my_l2 = v; my_n2 = hi; my_fl |= 2; dirty = true; }
          } else if (v <= my_l2) {               // second slot retired, everything else is >= l2 >= v
            my_l2 = v; my_n2 = hi; my_fl |= 2; dirty = true;
          } else {
            my_n2 = hi; my_fl &= ~2; dirty = true;       // l2 stays a lower bound of the rest
          }
        } else {
          dirty = true;
          if (!d2 && e2) {                       // nearest retired, the exact second takes over unless the union undercuts it
            if (v < my_l2) { my_l1 = v; my_n1 = hi; my_fl = 3; }
            else { my_l1 = my_l2; my_n1 = my_n2; my_n2 = hi; my_fl = 1; }
          } else {                               // only bounds left: exact iff the union is under the bound of the rest
            if (v <= my_l2) { my_l1 = v; my_n1 = hi; my_fl = 1; }
            else { my_l1 = my_l2; my_n1 = hi; my_fl = 0; }
            if (d2) my_n2 = hi;
          }
        }
      }
    }
  }
  // ---- (4) publish: the two smallest of the new / rescanned row's slice, the record of this workgroup's rows ----
  double b1, b2, rv;
  int bi1, bi2, rx;
  block_top2_min(pv, in ? z : 0x7fffffff, DINF, 0x7fffffff, (in && z != excl) ? my_l1 : DINF, in ? z : 0x7fffffff, b1, bi1, b2,
                 bi2, rv, rx, sval, sidx);
  if (t == 0) {
    StepPart2 p;
    p.v1 = b1; p.v2 = b2; p.i1 = bi1; p.i2 = bi2;
    part_out[w] = p;
  }
  if (z == rx) {          // rx is always a row of this workgroup (every thread contributes its own index)
    StepRec r;
    r.v = rv; r.x = rx; r.y = rv < DINF ? my_n1 : -1; r.exact = rv < DINF && (my_fl & 1) != 0 && my_n1 >= 0; r.pad = 0;
    rec_out[w] = r;
  }
  if (in && dirty) { l1a[z] = my_l1; l2a[z] = my_l2; n1a[z] = my_n1; n2a[z] = my_n2; fla[z] = my_fl; }
  if (in && sz_dirty) size[z] = my_sz;
}

#define LCHK(call)                                   \
  do {                                               \
    if ((call) != hipSuccess) { rc = DZN_E_HIP; goto done; } \
  } while (0)


// ---- the host stage's device context (r5) -----------------------------------------------------------------------------
// The clustering entry points below are called from the HOST stage of the pipeline, which (pipeline.diarize_many, bench.py)
// now runs in its own thread WHILE the engine executes the device stage of the next recording.  So they must not touch the
// legacy null stream (its copies and launches order themselves behind every kernel the engine has queued) and must not
// hipFree (a device-wide synchronisation: the host thread would sit out the engine's whole queue).  Per device:
//   * one non-blocking stream of the highest priority the device offers — the single-workgroup-per-256-rows step kernels are
//     latency bound, their workgroups are placed as soon as a CU of the engine's launches drains;
//   * one grow-only arena that every call carves its buffers from (re-allocated only when a call needs more than any before
//     it; dzn_host_workspace_release() returns it).  A mutex serialises the calls of one process.
struct HostCtx {
  hipStream_t stream = nullptr;
  char* base = nullptr;
  size_t cap = 0;
  char* sbase = nullptr;      // second arena: a STATE that lives across calls (vbx.hip), leased to one state at a time
  size_t scap = 0;
  bool sleased = false;
  hipEvent_t ev[2] = {nullptr, nullptr};      // created by the first dzn_link_speakers call on the device, kept with the stream
};
constexpr int MAX_DEV = 64;
std::mutex g_host_mu;
HostCtx g_host[MAX_DEV];

// the context of the CURRENT device with an arena of at least `bytes` (g_host_mu held)
int host_ctx(int device, size_t bytes, HostCtx** out) {
  int dev = device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return DZN_E_HIP;
  if (dev < 0 || dev >= MAX_DEV) return DZN_E_INVALID;
  HostCtx& c = g_host[dev];
  if (!c.stream) {
    int lo = 0, hi = 0;      // "least" and "greatest" priority: numerically greatest = lowest
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    if (hipStreamCreateWithPriority(&c.stream, hipStreamNonBlocking, hi) != hipSuccess) {
      c.stream = nullptr;
      return DZN_E_HIP;
    }
  }
  if (bytes == 0) {      // stream only
    *out = &c;
    return DZN_OK;
  }
  if (bytes > c.cap) {
    if (c.base) {
      (void)hipStreamSynchronize(c.stream);
      (void)hipFree(c.base);
      c.base = nullptr;
      c.cap = 0;
    }
    const size_t want = bytes + bytes / 8;      // a little headroom: recordings of one corpus differ by a few rows
    if (hipMalloc(&c.base, want) != hipSuccess) {
      (void)hipGetLastError();
      if (hipMalloc(&c.base, bytes) != hipSuccess) { (void)hipGetLastError(); c.base = nullptr; return DZN_E_NOMEM; }
      c.cap = bytes;
    } else {
      c.cap = want;
    }
  }
  *out = &c;
  return DZN_OK;
}

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(char* b) : base(b) {}
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

}  // namespace

int host_stage_stream(int device, hipStream_t* stream) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  HostCtx* c = nullptr;
  const int rc = host_ctx(device, 0, &c);
  if (rc == DZN_OK) *stream = c->stream;
  return rc;
}

int host_state_lease(int device, size_t bytes, hipStream_t* stream, char** base) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  HostCtx* c = nullptr;
  const int rc = host_ctx(device, 0, &c);
  if (rc != DZN_OK) return rc;
  *stream = c->stream;
  *base = nullptr;
  if (c->sleased) return DZN_OK;                 // a second live state: the caller allocates for itself
  if (bytes > c->scap) {
    if (c->sbase) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(c->sbase);
      c->sbase = nullptr;
      c->scap = 0;
    }
    if (hipMalloc(&c->sbase, bytes + bytes / 8) == hipSuccess) c->scap = bytes + bytes / 8;
    else {
      (void)hipGetLastError();
      if (hipMalloc(&c->sbase, bytes) != hipSuccess) { (void)hipGetLastError(); c->sbase = nullptr; return DZN_E_NOMEM; }
      c->scap = bytes;
    }
  }
  c->sleased = true;
  *base = c->sbase;
  return DZN_OK;
}

// gallery.hip: one call's hold on the context — the mutex from construction to destruction, the stream, and `bytes` of the
// per-call arena (the same discipline as the two entry points below, for a translation unit that cannot see HostCtx)
HostScratch::HostScratch(int device, size_t bytes) {
  g_host_mu.lock();
  HostCtx* c = nullptr;
  rc = host_ctx(device, bytes, &c);
  if (rc == DZN_OK) { stream = c->stream; base = bytes ? c->base : nullptr; }
}
HostScratch::~HostScratch() { g_host_mu.unlock(); }

void host_state_release(int device) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  int dev = device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return;
  if (dev >= 0 && dev < MAX_DEV) g_host[dev].sleased = false;
}

extern "C" int dzn_host_workspace_release(int32_t device) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  for (int dev = 0; dev < MAX_DEV; ++dev) {
    if (device >= 0 && dev != device) continue;
    HostCtx& c = g_host[dev];
    if (!c.base && !c.sbase && !c.stream) continue;
    DeviceGuard dg(dev);
    if (!dg.ok) return DZN_E_HIP;
    if (c.stream) (void)hipStreamSynchronize(c.stream);
    if (c.base) (void)hipFree(c.base);
    c.base = nullptr;
    c.cap = 0;
    if (c.sbase && !c.sleased) {      // a live state keeps its arena
      (void)hipFree(c.sbase);
      c.sbase = nullptr;
      c.scap = 0;
    }
  }
  return DZN_OK;
}

extern "C" int64_t dzn_host_workspace_bytes(int32_t device) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  return device >= 0 && device < MAX_DEV ? (int64_t)(g_host[device].cap + g_host[device].scap) : 0;
}

namespace {

struct LinkStats {      // the last dzn_link_speakers call of the process (g_host_mu held while written and read)
  int64_t launches = 0;     // step launches queued, surplus ones included
  int32_t merges = 0, rescans = 0;
  float pdist_ms = 0.f;     // the distance kernel alone, by HIP events
};
LinkStats g_link_stats;

// Both clustering entry points: upload, distance matrix, step loop under RULE, download.  RULE_CENTROID: euclidean distances,
// all n - 1 merges.  RULE_COMPLETE: masked cosine distances (h_group), the merges of height <= threshold, their number in
// *h_merges.
template <int RULE>
int run_linkage(const float* h_emb, const int32_t* h_group, int32_t n, int32_t dim, double threshold, double* h_Z,
                int32_t* h_merges, int32_t device) {
  int rc = DZN_OK;
  const int nblk = (n + LB_BLK - 1) / LB_BLK;
  std::vector<int> ones(n, 1), ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  DeviceGuard dg(device);      // restores the caller's device on every return path
  if (!dg.ok) return DZN_E_HIP;
  std::lock_guard<std::mutex> lk(g_host_mu);
  // the buffers of one call, carved from the arena (first pass: sizes only)
  float* E = nullptr;
  double *D = nullptr, *Z = nullptr, *l1a = nullptr, *l2a = nullptr, *nrm = nullptr;
  int *n1a = nullptr, *n2a = nullptr, *fla = nullptr, *size = nullptr, *cid = nullptr, *group = nullptr;
  StepState* st2 = nullptr;
  StepRec* rec2 = nullptr;
  StepPart2* part2 = nullptr;
  auto carve = [&](char* base) {
    Carver c(base);
    D = c.take<double>((size_t)n * n);
    E = c.take<float>((size_t)n * dim);
    l1a = c.take<double>(n);
    Z = c.take<double>((size_t)(n - 1) * 4);
    n1a = c.take<int>(n);
    size = c.take<int>(n);
    cid = c.take<int>(n);
    st2 = c.take<StepState>(2);
    rec2 = c.take<StepRec>((size_t)2 * nblk);
    fla = c.take<int>(n);      // keeps rec2 and part2, which every workgroup reads in every launch, n * 4 bytes apart
    part2 = c.take<StepPart2>((size_t)2 * nblk);
    l2a = c.take<double>(n);
    n2a = c.take<int>(n);
    if (RULE == RULE_COMPLETE) {
      nrm = c.take<double>(n);
      group = c.take<int>(n);
    }
    return c.off;
  };
  HostCtx* ctx = nullptr;
  rc = host_ctx(device, carve(nullptr), &ctx);
  if (rc != DZN_OK) return rc;
  carve(ctx->base);
  hipStream_t s = ctx->stream;
  int merges = 0;
  hipEvent_t* ev = ctx->ev;      // around the distance kernel of RULE_COMPLETE (dzn_link_speakers_last)
  const bool timed = RULE == RULE_COMPLETE && ((ev[0] && ev[1]) || (hipEventCreate(&ev[0]) == hipSuccess &&
                                                                    hipEventCreate(&ev[1]) == hipSuccess));
  LCHK(hipMemcpyAsync(E, h_emb, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, s));
  if (RULE == RULE_COMPLETE) LCHK(hipMemcpyAsync(group, h_group, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
  LCHK(hipMemcpyAsync(size, ones.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
  LCHK(hipMemcpyAsync(cid, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
  LCHK(hipMemsetAsync(st2, 0, 2 * sizeof(StepState), s));
  {
    const int tiles = (n + 63) / 64;
    if (RULE == RULE_COMPLETE) {
      hipLaunchKernelGGL(row_norm_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, E, n, dim, nrm);
      if (timed) LCHK(hipEventRecord(ev[0], s));
      hipLaunchKernelGGL(pdist_cosine_group_kernel, dim3(tiles, tiles), dim3(256), 0, s, E, nrm, group, n, dim, D);
      if (timed) LCHK(hipEventRecord(ev[1], s));
    } else {
      hipLaunchKernelGGL(pdist_kernel, dim3(tiles, tiles), dim3(256), 0, s, E, n, dim, D);
    }
    hipLaunchKernelGGL(init_rows2_kernel, dim3(n), dim3(256), 0, s, D, n, l1a, l2a, n1a, n2a, fla);
    hipLaunchKernelGGL(init_rec2_kernel, dim3(nblk), dim3(LB_BLK), 0, s, n, l1a, n1a, rec2);
    // one launch per step (merge or rescan); the number of rescans is data dependent, so launches are queued in
    // batches sized from the merges still missing and the step descriptor is read back between batches (surplus
    // launches after the last merge return at once)
    int64_t launched = 0;
    int remaining = n - 1;
    const auto t_loop = std::chrono::steady_clock::now();
    for (int round = 0; remaining > 0; ++round) {
      if (round > 64 + n) { rc = DZN_E_INVALID; goto done; }   // cannot happen: every batch completes >= 1 merge or stops
      // surplus launches return at once but still cost a kernel boundary each: size the batch for the expected rescans
      // (1.1-1.3 launches per merge) and let the next round finish the rest
      const int batch = remaining + remaining / 8 + 32;
      for (int i = 0; i < batch; ++i, ++launched)
        hipLaunchKernelGGL(step2_kernel<RULE>, dim3(nblk), dim3(LB_BLK), 0, s, D, n, l1a, l2a, n1a, n2a, fla, size, cid, Z, st2,
                           rec2, part2, (int)(launched & 1), threshold);
      LCHK(hipGetLastError());
      StepState hs;
      LCHK(hipMemcpyAsync(&hs, st2 + (launched & 1), sizeof(StepState), hipMemcpyDeviceToHost, s));
      LCHK(hipStreamSynchronize(s));
      if (hs.kind == STEP_FAIL) { rc = DZN_E_INVALID; goto done; }   // non-finite distances
      remaining = hs.kind == STEP_DONE ? 0 : n - 1 - hs.k;           // (RULE_COMPLETE: also the stop at the threshold)
      merges = hs.k;
      if (remaining == 0 && RULE == RULE_COMPLETE) {
        g_link_stats.launches = launched;
        g_link_stats.merges = hs.k;
        g_link_stats.rescans = hs.pad;
      }
      if (remaining == 0 && getenv("DZN_LINKAGE_DEBUG"))
        fprintf(stderr, "linkage[two neighbours%s]: n %d, %lld launches in %d batches, %d rescans, loop %.1f ms, %d merges\n",
                RULE == RULE_COMPLETE ? ", complete" : "", n, (long long)launched, round + 1, hs.pad,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop).count(), hs.k);
    }
  }
  LCHK(hipGetLastError());
  if (RULE == RULE_CENTROID) merges = n - 1;
  if (merges > 0) LCHK(hipMemcpyAsync(h_Z, Z, (size_t)merges * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (h_merges) *h_merges = merges;
done:
  // the host vectors above (ones, ids) are sources of queued copies; an asynchronous fault of a step kernel or of the final
  // copy surfaces HERE, and h_Z is garbage then: it must not return DZN_OK
  if (hipStreamSynchronize(s) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;
  if (RULE == RULE_COMPLETE) {
    g_link_stats.pdist_ms = 0.f;
    if (rc == DZN_OK && timed && hipEventElapsedTime(&g_link_stats.pdist_ms, ev[0], ev[1]) != hipSuccess)
      g_link_stats.pdist_ms = 0.f;
  }
  return rc;
}

}  // namespace

extern "C" int dzn_linkage_centroid(const float* h_emb, int32_t n, int32_t dim, double* h_Z, int32_t device) {
  if (!h_emb || !h_Z || n < 2 || dim < 1) return DZN_E_INVALID;
  return run_linkage<RULE_CENTROID>(h_emb, nullptr, n, dim, 0.0, h_Z, nullptr, device);
}

extern "C" int dzn_link_speakers(const float* h_emb, const int32_t* h_group, int32_t n, int32_t dim, double threshold,
                                 double* h_Z, int32_t* h_merges, int32_t device) {
  if (!h_emb || !h_group || !h_Z || !h_merges || n < 2 || dim < 1) return DZN_E_INVALID;
  if (!(threshold > 0.0 && threshold <= 2.0)) return DZN_E_INVALID;      // (NaN compares false)
  for (int64_t r = 0; r < n; ++r) {      // a row that is all zero or not finite has no direction: refused before any upload
    const float* e = h_emb + r * dim;
    bool any = false;
    for (int c = 0; c < dim; ++c) {
      if (!isfinite(e[c])) return DZN_E_INVALID;
      any |= e[c] != 0.f;
    }
    if (!any) return DZN_E_INVALID;
  }
  return run_linkage<RULE_COMPLETE>(h_emb, h_group, n, dim, threshold, h_Z, h_merges, device);
}

extern "C" int dzn_link_speakers_last(int64_t* launches, int32_t* merges, int32_t* rescans, float* pdist_ms) {
  std::lock_guard<std::mutex> lk(g_host_mu);
  if (launches) *launches = g_link_stats.launches;
  if (merges) *merges = g_link_stats.merges;
  if (rescans) *rescans = g_link_stats.rescans;
  if (pdist_ms) *pdist_ms = g_link_stats.pdist_ms;
  return DZN_OK;
}

// ---- cosine distances of every embedding to the cluster centroids (row f1: `cdist` of the assignment step) -------
// scipy.spatial.distance.cdist(E, Cn, metric="cosine") of BaseClustering.assign_embeddings
// (PA/pipelines/clustering.py:207-216): float64, row norms first, then per pair
//     d = 1 - clip(dot(u, v) / (|u| |v|))
// The kernels below use the same formula in float64 with in-order sums and separate product / sum roundings
// (contraction off), one thread per (row[, centroid]) walking the 256 dimensions, so identical rows give identical
// scores (ties stay ties).  scipy's own summation order is its build's: measured agreement 2e-15 on distances of
// order 1 (tests/test_ops_gpu.py), i.e. the level at which scipy differs from a plain in-order loop.  72 k
// embeddings x 13 centroids at 4 h of audio is 0.24 G flop in float64 — the point is the 0.3-0.7 s scipy spends
// converting and scanning 147 MB on one host core.
namespace {

__global__ __launch_bounds__(256) void row_norm_f64_kernel(const double* __restrict__ X, int n, int dim,
                                                           double* __restrict__ nrm) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const double* x = X + (int64_t)r * dim;
  double s = 0.0;
  for (int i = 0; i < dim; ++i) {
    const double p = x[i] * x[i];
    s = s + p;
  }
  nrm[r] = sqrt(s);
}

// thread -> (row, centroid) with the centroid fastest: the lanes of a wavefront share a handful of rows
__global__ __launch_bounds__(256) void cdist_cosine_kernel(const float* __restrict__ E, const double* __restrict__ Cn,
                                                           const double* __restrict__ ne, const double* __restrict__ nc,
                                                           int n, int dim, int k, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n * k) return;
  const int r = (int)(idx / k), c = (int)(idx - (int64_t)r * k);
  const float* e = E + (int64_t)r * dim;
  const double* v = Cn + (int64_t)c * dim;
  double s = 0.0;
  for (int i = 0; i < dim; ++i) {
    const double p = (double)e[i] * v[i];
    s = s + p;
  }
  const double den = ne[r] * nc[c];
  double cosine = s / den;
  if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);      // scipy clips the rounding error
  out[idx] = 1.0 - cosine;
}

}  // namespace

extern "C" int dzn_cdist_cosine(const float* h_emb, int32_t n, int32_t dim, const double* h_cent, int32_t k,
                                double* h_dist, int32_t device) {
  if (!h_emb || !h_cent || !h_dist || n < 1 || dim < 1 || k < 1) return DZN_E_INVALID;
  int rc = DZN_OK;
  DeviceGuard dg(device);      // restores the caller's device on every return path
  if (!dg.ok) return DZN_E_HIP;
  std::lock_guard<std::mutex> lk(g_host_mu);       // own stream + arena: see "the host stage's device context" above
  float* E = nullptr;
  double *Cn = nullptr, *ne = nullptr, *nc = nullptr, *D = nullptr;
  auto carve = [&](char* base) {
    Carver c(base);
    E = c.take<float>((size_t)n * dim);
    Cn = c.take<double>((size_t)k * dim);
    ne = c.take<double>(n);
    nc = c.take<double>(k);
    D = c.take<double>((size_t)n * k);
    return c.off;
  };
  HostCtx* ctx = nullptr;
  rc = host_ctx(device, carve(nullptr), &ctx);
  if (rc != DZN_OK) return rc;
  carve(ctx->base);
  hipStream_t s = ctx->stream;
  LCHK(hipMemcpyAsync(E, h_emb, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, s));
  LCHK(hipMemcpyAsync(Cn, h_cent, (size_t)k * dim * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(row_norm_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, E, n, dim, ne);
  hipLaunchKernelGGL(row_norm_f64_kernel, dim3((k + 255) / 256), dim3(256), 0, s, Cn, k, dim, nc);
  hipLaunchKernelGGL(cdist_cosine_kernel, dim3((unsigned)(((int64_t)n * k + 255) / 256)), dim3(256), 0, s, E, Cn, ne, nc,
                     n, dim, k, D);
  LCHK(hipGetLastError());
  LCHK(hipMemcpyAsync(h_dist, D, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, s));
done:
  if (hipStreamSynchronize(s) != hipSuccess && rc == DZN_OK) rc = DZN_E_HIP;   // h_dist is only valid after a clean drain
  return rc;
}
