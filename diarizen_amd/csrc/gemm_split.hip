// gemm_split.hip — fp32 contraction on the bf16 matrix pipe: exact 3-way operand split
// ("f32s" engine mode, DZN_PREC_F32_SPLIT).
//
// Every fp32 value x is written as x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi),
// lo = bf16(x - hi - mid) (round-to-nearest at each level; the two subtractions are exact and
// lo needs <= 8 significant bits, so the decomposition is EXACT).  A product a*w is then
//     a_hi w_hi + (a_hi w_mid + a_mid w_hi) + (a_hi w_lo + a_mid w_mid + a_lo w_hi)  [+ O(2^-24) terms]
// i.e. six v_mfma_f32_16x16x32_bf16 products accumulated in fp32; the three dropped cross terms
// (mid*lo, lo*mid, lo*lo) are bounded by 2^-22 |a w| — the size of one or two fp32 roundings of the
// product.  6 bf16 MFMAs of 16 cycles replace 8 fp32 MFMAs (16x16x4) of 32 cycles for the same
// 16x16x32 block: 2.67x less matrix-pipe time at fp32-grade accuracy (tests/test_ops_gpu.py
// measures both kernels against a float64 product).
//
// Same contract as gemm.hip (dzn_gemm_desc, fused epilogue).  Data movement:
//   A (activations) : fp32 in HBM, fp32 tile in LDS by LDS-DMA (128-B rows, XOR-swizzled exactly
//       like the fp32 kernel); each wavefront splits the fragments it reads in registers
//       (v_cvt_pk_bf16_f32 / shifts / packed fp32 subtracts, overlapped with the MFMAs).
//   W (weights)     : split ONCE when the weights are packed (dzn_op_split_weights) into
//       [N][K/32][plane 3][32] bf16; the 32 k of a block are stored in the order the fragment
//       reads want (lane group q owns k = 4q..4q+3 and 16+4q..16+4q+3, matching the two 16-B
//       slots q and 4+q of the fp32 A row), so every fragment is one ds_read_b128.  Each plane
//       of a W tile is a [BN][64 B] LDS image; slot s of row r is stored at s ^ g((r>>2)&3),
//       g = (0,2,3,1), which makes the four 16-lane groups of ds_read_b128 conflict free.
// Requires K % 32 == 0 and kc % 32 == 0 (else the caller falls back to the fp32 MFMA kernel).
//
// NP = 2 ("f32h", DZN_PREC_F32_H2): the same kernel with a TWO-term fp16 split and THREE products
// (hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16) — the error-corrected tensor-core scheme of Ootomo &
// Yokota (and of "3xTF32": fp16 and TF32 both carry 11 significant bits).  x*s = hi + lo + r with
// hi = fp16(x*s), lo = fp16(x*s - hi), |r| <= 2^-22 |x*s|; the dropped terms (lo*lo and the two residuals) are
// <= 3 * 2^-22 |a w| — the size of a few fp32 roundings of the product — and half the matrix-pipe work of
// NP = 3.  fp16's 5-bit exponent is handled by EXACT power-of-two scaling on both sides: the weights are
// scaled per output row when they are split (max |w| of the row lands in [2^14, 2^15), dzn_op_split_weights_h2),
// the activations by s = 2^(14 - floor(log2 amax)) from the running |max| the PRODUCER of the tensor tracked
// (dzn_gemm_desc.a_amax / c_amax); the epilogue multiplies the accumulator by the exact inverse powers of two.
// Elements more than 2^17 below the tensor's maximum keep a lo term in fp16's subnormal range: their ABSOLUTE
// error stays <= 2^-25 * max / 2^14, i.e. below fp32 resolution of any dot product that contains the maximum.
#include <cmath>
#include <type_traits>

#include "checked.h"
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_launch.h"
#include "split.h"

DZN_CHECKED_TU(gemm_split)

namespace {

__device__ __forceinline__ int wswz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }

// s_waitcnt vmcnt(N) lgkmcnt(0), expcnt left at its maximum (gfx9 encoding: vmcnt = [3:0] + [15:14])
template <int N>
__device__ __forceinline__ void wait_vm_lgkm0() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4));
}

// the second A segment's row table (BM x 4 bytes) rides in LDS unless it would push one of the OCC resident workgroups out
constexpr bool a2_tab_in_lds(int stage_bytes, int BM, int OCC) { return (stage_bytes + BM * 4) * OCC <= 160 * 1024; }

// BM x BN tile per workgroup of WGM x WGN wavefronts, S LDS stages of one 32-k tile each.
//
// Pipeline.  The matrix pipe retires a K tile in ~1.5k cycles per wavefront-tile while an LDS-DMA
// fill needs 1.1-1.7 us (2.6k-4k cycles) to land, and a wavefront that has just passed a barrier
// needs ~0.5k cycles of ds_read + split before its first MFMA.  So:
//   * tiles are prefetched S tiles ahead (raw s_barrier + s_waitcnt vmcnt(N) that leaves the
//     younger tiles in flight; __syncthreads would drain them);
//   * the barrier of K tile kt sits in the MIDDLE of the tile's MFMAs: the first half of the
//     rows is multiplied, then [wait tile kt+1, barrier, refill the stage of tile kt], then the
//     fragments of tile kt+1 are read into the second register set while the second half of
//     tile kt is multiplied — the matrix pipe has work queued across the barrier.
template <int BM, int BN, int WGM, int WGN, int S, int NP, int OCC = 1>
__global__ __launch_bounds__(WGM * WGN * 64, OCC) void gemm_split_kernel(const dzn_gemm_desc d) {
  constexpr int NW = WGM * WGN;           // wavefronts per workgroup
  constexpr int BK = 32;
  constexpr int TM = BM / WGM, TN = BN / WGN;
  constexpr int MI = TM / 16, NI = TN / 16, MH = MI / 2;
  constexpr int RB = NW * 1024;           // bytes per LDS-DMA round (1 KiB per wavefront)
  constexpr int ACH = BM * 128 / RB;      // rounds of the A tile (BM rows x 128 B)
  constexpr int WROWS = NW * 16;          // rows of one W plane per round (64-B rows)
  constexpr int WR = (BN + WROWS - 1) / WROWS;
  constexpr int SP = NP == 3 ? 3 : 2;     // planes STORED per weight row (NP = 1 reads the leading one of two)
  constexpr int ABYTES = BM * 128, WPLANE = BN * 64, BUF = ABYTES + NP * WPLANE;
  constexpr int LPT = ACH + NP * WR;      // LDS-DMA instructions per thread per tile (NP fewer for the
                                          // wavefronts that sit out a partial last W round)
  constexpr bool WPART = BN % WROWS != 0;
  constexpr bool A2_TAB_LDS = a2_tab_in_lds(S * BUF, BM, OCC);
  static_assert(BM * 128 % RB == 0, "A tile must be whole rounds");
  static_assert(MI % 2 == 0, "two row halves per wavefront tile");
  static_assert(S >= 2 && (S - 1) * LPT < 64, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: LDS-DMA bases stay scalar
  const int wm = wave / WGN, wn = wave % WGN;
  // the tiles are walked XCD by XCD (contiguous ranges) in row-block-major order: an XCD works on a few row blocks with ALL their
  // column tiles, so it streams the whole weight-plane set (N x K x 2 NP bytes) once per row block.  From ~4 MB on that set no
  // longer survives in the XCD's 4 MB L2 between two row blocks, but the re-fetched planes come from the Infinity Cache at no
  // measurable cost in time: a group-major order that cut the fabric reads as modelled left the step unchanged and was removed
  // (DESIGN.md §5 "Switch retirement", profiles/r4_gemm_refetch_probe.txt).
  const int tilesN = (d.N + BN - 1) / BN;
  int tm, tn, z0, z1;
  if (!gemm_tile(d, tilesN, tm, tn, z0, z1)) return;
  const float* __restrict__ A = d.A + z0 * d.a_z0 + z1 * d.a_z1;
  const u16* __restrict__ W3 =
      reinterpret_cast<const u16*>(NP == 3 ? d.W3 : d.W2h) + SP * (z0 * d.w_z0 + z1 * d.w_z1);
  // NP = 2: exact power-of-two scale of every A row from the |max| tracker of the UNIT (window / image) the row
  // belongs to — unit = m / amax_unit, or the z batch index when amax_unit == 0 — so that a window's result does
  // not depend on what else is in the batch
  float a_scale[MI], row_inv[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_scale[i] = row_inv[i] = 1.f;
  if constexpr (NP <= 2) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      int m = tm * BM + wm * TM + i * 16 + (lane & 15);
      m = m < d.M ? m : d.M - 1;
      const int unit = d.amax_unit > 0 ? m / d.amax_unit : z0;
      DZN_CHECK(d.amax_count <= 0 || (unit >= 0 && unit < d.amax_count), 0x101, unit);   // tracker index inside its array
      // two sources (dzn_gemm_desc.A2): ONE scale for both segments, from the larger of the two bounds
      float am = d.a_amax[unit];
      if (d.A2) am = fmaxf(am, d.a2_amax[unit]);
      h2_scale(am, a_scale[i], row_inv[i]);
    }
  }
  const int64_t cz = z0 * d.c_z0 + z1 * d.c_z1;
  const int64_t bz = z0 * d.b_z0 + z1 * d.b_z1;

  // A: thread -> (row = tid/8 + 8 NW i, physical slot tid%8), logical chunk = slot ^ ((row>>1)&7)
  const int r0 = tid >> 3;
  const int csw = (tid & 7) ^ ((r0 >> 1) & 7);
  const float* aptr[ACH];   // per-thread source of K tile 0; a K tile adds a uniform offset
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    int m = tm * BM + r0 + 8 * NW * i;
    m = m < d.M ? m : d.M - 1;
    aptr[i] = A + (d.a_rowoff ? (int64_t)d.a_rowoff[m] : (int64_t)m * d.lda) + csw * 4;
  }
  // second A segment (dzn_gemm_desc.A2): the row table of this tile's BM rows waits in LDS behind the stages, so the K loop
  // carries no second set of row pointers; the first barrier publishes it (k1 >= 128: no prologue tile is past k1).  Where
  // those BM x 4 bytes would cost a resident workgroup (three bf16 planes of a 128 x 128 tile fill the LDS exactly) the rows
  // are read from the table in memory at the switch instead.
  int* a2tab = reinterpret_cast<int*>(smem + S * BUF);
  if (A2_TAB_LDS && d.A2 && tid < BM) {
    int m = tm * BM + tid;
    m = m < d.M ? m : d.M - 1;
    a2tab[tid] = d.a2_rowoff[m];
  }
  // W planes: thread -> (row = 16 wave + lane/4 + 16 NW i, physical slot lane%4); rows past N re-read
  // row N-1 (their accumulators are never stored); a partial last round is fetched by the first waves only
  const bool wfull = !WPART || (WR - 1) * WROWS + wave * 16 < BN;   // wave-uniform
  const int wr0 = wave * 16 + (lane >> 2);
  const int wsw = (lane & 3) ^ wswz(wr0);
  const u16* wptr[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    int n = tn * BN + wr0 + WROWS * i;
    n = n < d.N ? n : d.N - 1;
    wptr[i] = W3 + (int64_t)n * SP * d.ldw + wsw * 8;
  }

  // the next K tile to fetch: k index and its A element offset (two-level K addressing), advanced
  // incrementally on the scalar unit
  int ik = 0, irem = 0;
  int64_t ikoff = 0;
  auto issue = [&](int stage) {
    unsigned char* sA = smem + stage * BUF + wave * 1024;
    unsigned char* sW = smem + stage * BUF + ABYTES + wave * 1024;
    DZN_CHECK(stage >= 0 && stage < S && ik < d.K, 0x102, stage);                              // a stage of the ring, a k tile of the operand
    DZN_CHECK(wave * 1024 + (ACH - 1) * RB + 1024 <= ABYTES, 0x103, wave);                      // A fill stays inside the A image
    DZN_CHECK(!wfull || wave * 1024 + (WR - 1) * RB + 1024 <= WPLANE, 0x104, wave);                  // W fill stays inside its plane image
    if (d.A2 && ik == d.k1) {   // tile-uniform, once per workgroup: from this K tile on the rows come from the second source
      const float* A2 = d.A2 + z0 * d.a2_z0;
#pragma unroll
      for (int i = 0; i < ACH; ++i) {
        int off;
        if constexpr (A2_TAB_LDS) {
          off = a2tab[r0 + 8 * NW * i];
        } else {
          int m = tm * BM + r0 + 8 * NW * i;
          off = d.a2_rowoff[m < d.M ? m : d.M - 1];
        }
        aptr[i] = A2 + off + csw * 4;
      }
      ikoff = 0;
      irem = -(1 << 30);        // one run of k2 columns: the two-level wrap never fires again
    }
#pragma unroll
    for (int i = 0; i < ACH; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(aptr[i] + ikoff),
                                       (__attribute__((address_space(3))) void*)(sA + i * RB), 16, 0, 0);
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int i = 0; i < WR; ++i)
        if (i + 1 < WR || wfull)
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(wptr[i] + SP * ik + p * 32),
              (__attribute__((address_space(3))) void*)(sW + p * WPLANE + i * RB), 16, 0, 0);
    ik += BK;
    irem += BK;
    ikoff += BK;
    if (irem == d.kc) { irem = 0; ikoff += d.ldk - d.kc; }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int lr = lane & 15, lq = lane >> 4;

  // per-lane LDS byte offsets of the fragments inside a stage
  int woff[NI], aoff0[MI], aoff1[MI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int row = wn * TN + j * 16 + lr;
    woff[j] = ABYTES + row * 64 + ((lq ^ wswz(row)) << 4);
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = wm * TM + i * 16 + lr;
    const int sw = (row >> 1) & 7;
    aoff0[i] = row * 128 + ((lq ^ sw) << 4);
    aoff1[i] = row * 128 + (((4 + lq) ^ sw) << 4);
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) DZN_CHECK(woff[j] >= ABYTES && woff[j] + (NP - 1) * WPLANE + 16 <= BUF, 0x105, woff[j]);   // fragment reads inside the stage
#pragma unroll
  for (int i = 0; i < MI; ++i) DZN_CHECK(aoff0[i] + 16 <= ABYTES && aoff1[i] + 16 <= ABYTES, 0x106, aoff1[i]);
  DZN_CHECK(tm * BM < d.M && tn * BN < d.N, 0x107, tm * tilesN + tn);                              // the tile exists
  auto read_w = [&](int stage, u32x4 (&wf)[NI][NP]) {
    const unsigned char* base = smem + stage * BUF;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int p = 0; p < NP; ++p) wf[j][p] = *reinterpret_cast<const u32x4*>(base + p * WPLANE + woff[j]);
  };
  auto read_a = [&](int stage, f32x4 (&ar)[MI][2]) {
    const unsigned char* base = smem + stage * BUF;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      ar[i][0] = *reinterpret_cast<const f32x4*>(base + aoff0[i]);
      ar[i][1] = *reinterpret_cast<const f32x4*>(base + aoff1[i]);
    }
  };
  // the products of one 16-row block against all NI column blocks: smallest terms first, NI independent
  // accumulators between dependent MFMAs.  af[] = A terms (hi, [mid,] lo), wf[j][] = W planes (hi, [mid,] lo).
  auto mma = [&](int i, const u32x4 (&wf)[NI][NP], const u32x4 (&af)[NP]) {
    if constexpr (NP == 3) {
      constexpr int PW[6] = {2, 0, 1, 1, 0, 0}, PA[6] = {0, 2, 1, 0, 1, 0};   // lo*hi hi*lo mid*mid mid*hi hi*mid hi*hi
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma_np<NP>(wf[j][PW[t]], af[PA[t]], acc[i][j]);
    } else if constexpr (NP == 2) {
      constexpr int PW[3] = {1, 0, 0}, PA[3] = {0, 1, 0};                     // lo*hi hi*lo hi*hi
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma_np<NP>(wf[j][PW[t]], af[PA[t]], acc[i][j]);
    } else {                                                                  // hi*hi (DZN_PREC_F16)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = mfma_np<NP>(wf[j][0], af[0], acc[i][j]);
    }
  };
  auto split = [&](const f32x4 (&a)[2], u32x4 (&af)[NP], float sc) {
    if constexpr (NP == 3) {
      bf16x8 h_, m_, l_;
      split8(a[0], a[1], h_, m_, l_);
      af[0] = __builtin_bit_cast(u32x4, h_);
      af[1] = __builtin_bit_cast(u32x4, m_);
      af[2] = __builtin_bit_cast(u32x4, l_);
    } else if constexpr (NP == 2) {
      split8_h2(a[0], a[1], sc, af[0], af[1]);
    } else {
      cvt8_h1(a[0], a[1], sc, af[0]);
    }
  };

  // two segments: the loop ends at k1 + k2 — the zero-padded weight columns behind it are neither fetched nor multiplied
  const int nk = (d.A2 ? d.k1 + d.k2 : d.K) / BK;
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s < nk) issue(s);
  // wait until all but the `T` youngest tiles of this wavefront's LDS-DMA have landed
  auto wait_tiles = [&](auto tiles) {
    constexpr int T = decltype(tiles)::value;
    if (wfull) wait_vm_lgkm0<T * LPT>();
    else wait_vm_lgkm0<T * (LPT - NP)>();
  };
  if (nk >= S) wait_tiles(std::integral_constant<int, S - 1>{});
  else wait_vm_lgkm0<0>();
  __builtin_amdgcn_s_barrier();
  u32x4 wfa[NI][NP], wfb[NI][NP];
  f32x4 ar[MI][2];
  read_w(0, wfa);
  read_a(0, ar);
  int stage = 0;

  // one K tile: `wc` holds its W fragments, `ar` its raw A fragments; leaves tile kt+1 in (wn_, ar)
  auto step = [&](int kt, const u32x4 (&wc)[NI][NP], u32x4 (&wn_)[NI][NP]) {
    const bool more = kt + 1 < nk;
#pragma unroll
    for (int i = 0; i < MH; ++i) {
      u32x4 af[NP];
      split(ar[i], af, a_scale[i]);
      mma(i, wc, af);
    }
    u32x4 af2[MI - MH][NP];
#pragma unroll
    for (int i = MH; i < MI; ++i) split(ar[i], af2[i - MH], a_scale[i]);
    const int nstage = stage + 1 == S ? 0 : stage + 1;
    __builtin_amdgcn_sched_barrier(0);  // keep the second half of the MFMAs BEHIND the barrier block
    if (more) {
      // tile kt+1 landed (tiles kt+2 .. kt+S-1 may stay in flight); all my reads of tile kt retired
      if (kt + S <= nk) wait_tiles(std::integral_constant<int, S - 2>{});
      else wait_vm_lgkm0<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + S < nk) issue(stage);  // every wave is past its reads of tile kt
      read_w(nstage, wn_);
      read_a(nstage, ar);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = MH; i < MI; ++i) mma(i, wc, af2[i - MH]);
    stage = nstage;
  };
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, wfa, wfb);
    if (kt + 1 < nk) step(kt + 1, wfb, wfa);
  }
  // the epilogue's column vectors live in LDS (48 registers less than holding them): the stages are dead once every
  // wavefront left the loop
  __syncthreads();
  gemm_epilogue<BM, BN, TM, TN, MI, NI, true>(d, acc, tm, tn, wm, wn, lr, lq, cz, bz, z0, row_inv, NP <= 2 ? d.col_scale : nullptr,
                                              reinterpret_cast<float*>(smem) + wave * 3 * TN);
}

// (r4) The same contraction on 32x32x16 MFMA blocks measured 253-272 TFLOP/s against 285-305 for the 16x16x32
// tile above and lost 4 % on the step; it was removed (profiles/r4_gemm_m32_probe.txt).

template <int BM, int BN, int WGM, int WGN, int S, int NP, int OCC = 1>
int launch_split_cfg(const dzn_gemm_desc& d, hipStream_t s, const char* tag = nullptr) {
  size_t lds = (size_t)S * (BM * 128 + NP * BN * 64);
  if (d.A2 && a2_tab_in_lds((int)lds, BM, OCC)) lds += BM * 4;   // + the second segment's row table
  if (!tag) tag = NP == 3 ? "f32s" : NP == 2 ? "f32h" : "f16";
  return launch_contraction<gemm_split_kernel<BM, BN, WGM, WGN, S, NP, OCC>>(d, s, WGM * WGN * 64, lds, BM, BN, WGN, tag, NP * 2);
}

// W [rows][K] fp32 (row stride ldw)  ->  W3 [rows][K/32][3][32] bf16, k permuted inside each block
__global__ __launch_bounds__(256) void split_weights_kernel(const float* __restrict__ W, int64_t rows, int K,
                                                            int64_t ldw, u16* __restrict__ W3) {
  const int64_t n = rows * K;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / K;
    const int k = (int)(i - r * K);
    const float x = W[r * ldw + k];
    const __bf16 h = (__bf16)x;
    const float r1 = x - (float)h;
    const __bf16 m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    const __bf16 l = (__bf16)r2;
    const int kk = k & 31;
    const int pos = 8 * ((kk & 15) >> 2) + (kk & 3) + 4 * (kk >> 4);
    u16* o = W3 + r * 3 * K + (int64_t)(k >> 5) * 96 + pos;
    o[0] = *reinterpret_cast<const u16*>(&h);
    o[32] = *reinterpret_cast<const u16*>(&m);
    o[64] = *reinterpret_cast<const u16*>(&l);
  }
}

template <int NP>
int launch_gemm_split_np(const dzn_gemm_desc& d, hipStream_t s) {
  if (const char* force = g_gemm_cfg.get()) {            // tuning knob: force one tile shape
    // production tiles by name
    if (!strcmp(force, "128x64")) return launch_split_cfg<128, 64, 4, 1, 2, NP, NP <= 2 ? 3 : 2>(d, s);
    if (!strcmp(force, "128x80")) return launch_split_cfg<128, 80, 4, 1, 2, NP, 2>(d, s);
    if (!strcmp(force, "128x32")) return launch_split_cfg<128, 32, 4, 1, 2, NP>(d, s);
    // (r5 probes, measured negative and removed: 64x64 tiles of 2 wavefronts, 128x32 at 4 workgroups per CU, a first-round stagger of
    //  the narrow tile — profiles/r5_short_k_probes.txt, code at commit 2a14565)
    if constexpr (NP == 3) {
      if (!strcmp(force, "128x128")) return launch_split_cfg<128, 128, 2, 2, 2, NP, 2>(d, s);
    } else {
      if (!strcmp(force, "128x128w4")) return launch_split_cfg<128, 128, 4, 1, 2, NP, 2>(d, s);
    }
    // (short-K probes at NP = 2, measured behind 128x128w4 at every K = 128 .. 512 and removed: 128 x 256 tiles of 4 x 2 wavefronts and
    //  256 x 128 tiles of 8 x 1, one 512-thread workgroup per CU, 96 KB of LDS — profiles/short_k_wide_probe.txt)
    if constexpr (NP == 1) {
      if (!strcmp(force, "256x128w8s3")) return launch_split_cfg<256, 128, 8, 1, 3, NP, 2>(d, s);
    }
  }
  // (r3's 8-wavefront ping-pong forms — gemm_pp.hip, 256 x 192 tiles — measured +0.5 % on the step and were removed in r4;
  // the A/B record is profiles/r3_gemm_pq_probe.txt, the source is in the history at 7bb9ad7)
  // (r4, all bit-identical, all measured neutral or negative, sources in the history: a separate three-stage A ring — aea83fd,
  // profiles/r4_gemm_a3_probe.txt; persistent workgroups with the next tile's prologue fill under the epilogue — 6ff2eda,
  // profiles/r4_gemm_persist_probe.txt; 256 x 256 tiles at one wavefront per SIMD — e863011, profiles/r4_gemm_wide_probe.txt,
  // whose PMC pass shows clock x matrix-pipe-busy constant across both forms: the K loop sits on a power-limited MFMA rate)
  // launch bounds pin the occupancy the tile was tuned at (r3: the pipelined epilogue gives the register allocator
  // room to trade occupancy for more loads in flight; 128x64 tiles want 3 workgroups per CU, 128x128 two)
  constexpr int OCC64 = NP <= 2 ? 3 : 2;
  if (d.N <= 32) return launch_split_cfg<128, 32, 4, 1, 2, NP>(d, s);
  const int cols128 = (d.N + 127) / 128 * 128, cols64 = (d.N + 63) / 64 * 64;
  // Short K on wide outputs (NP = 2, N >= 512, 128 <= K <= 512: the out-projections and the narrow FFN-down launches of the
  // pruned encoder, 44 launches per forward of the large model): the 128 x 128 tile of 4 x 1 wavefronts — the SAME kernel as the
  // K > 512 class below — under a profiler class of its own, gemm_f32h_sk_128x128, so that gemm_f32h_128x128 stays the
  // homogeneous long-K class of the roofline line.  Isolated sweep at 223839 x 1024 (profiles/short_k_wide_probe.txt): 7-15 %
  // below the 128 x 64 tile at every K from 128 (514 vs 607 us) to 512 (967 vs 1054 us), no crossover; 128 x 256 and
  // 256 x 128 tiles (one 512-thread workgroup per CU) lie between the two and were removed.  A/B on the step:
  // profiles/short_k_wide_ab.txt.  (r3 had measured 4-7 % in isolation with the step unmoved inside a +-1 % noise,
  // profiles/r3_tile_choice_short_k.txt.)
  // The rule reads N, K and NP only — never M, nz or stat_partial: a LayerNorm partial is the sum over ONE wavefront tile's
  // columns, so a tile that followed M would make a window's float outputs depend on its batch (see the 448-workgroup rule
  // below).  At N = 1024 these launches now leave 8 partials per row instead of 16.  Widths whose last 128-wide tile would be
  // mostly padding stay narrow, by the same 1/8 test as for long K.  K < 128 (the heavily pruned layers, ~6 ms of the step)
  // and N < 512 stay on the narrow tile: they were not measured.
  if constexpr (NP == 2)
    if (d.N >= 512 && d.K >= 128 && d.K <= 512 && cols64 * 9 >= cols128 * 8)
      return launch_split_cfg<128, 128, 4, 1, 2, NP, 2>(d, s, "f32h_sk");
  // 128x64 tiles run 4 wavefronts as 4x1 (32 rows x 64 columns each): the in-register operand
  // split is per A row, so wide-and-short wavefront tiles halve the VALU work per MFMA
  // (r5) requesting the residual of short-K launches at kernel start cost the third workgroup per CU (class 168 -> 134 TFLOP/s) and
  // was removed: DESIGN.md §4.9, profiles/r5_rpf_probe.txt
  if (d.N <= 64 || d.K <= 512) return launch_split_cfg<128, 64, 4, 1, 2, NP, OCC64>(d, s);
  // 128-wide column tiles unless 64-wide ones save more than ~1/8 of the (padded) columns; widths that
  // are multiples of 80 but not of 64 (conv1 of the extractor: 153 -> 160) get exact 80-wide tiles
  // small launches (BASELINE configs[1]: 32 windows of 5 s = 7968 rows): 128 x 128 tiles would leave most of the 512
  // workgroup slots (256 CUs x 2) empty — halve the tile so that twice as many workgroups exist
  // A launch that leaves LayerNorm partials (stat_partial) is exempt: a partial is the sum over ONE wavefront tile's columns, so
  // the tile width decides how a row's statistics are added up, and with this rule it would follow M — the float outputs of a
  // window (log-probabilities, soft scores) would depend on how many windows share its batch (17 or fewer windows of 8 s took
  // the narrow tile, 18 or more the wide one).  The u8 decisions never showed it; the live scores compare
  // floats of windows run one by one with those of a whole recording.
  if (!d.stat_partial && (int64_t)((d.M + 127) / 128) * (cols128 / 128) * (d.nz > 0 ? d.nz : 1) < 448)
    return launch_split_cfg<128, 64, 4, 1, 2, NP, OCC64>(d, s);
  if (d.N % 80 == 0 && d.N < cols64 && d.N * 9 < cols128 * 8) return launch_split_cfg<128, 80, 4, 1, 2, NP, 2>(d, s);
  if (cols64 * 9 < cols128 * 8) return launch_split_cfg<128, 64, 4, 1, 2, NP, OCC64>(d, s);
  // NP = 2: 4 x 1 wavefronts (32 x 128 each): every A row is split by ONE wavefront instead of two; measured +3 %
  // over 2 x 2 on the pipeline's K = 1024 shapes (scripts/bench_gemm_h2.py).  NP = 3 keeps 2 x 2 (register budget).
  // NP = 1 (DZN_PREC_F16) is bound by the global -> LDS fill, not by MFMA / VALU (ablation: profiles/r2_gemm_ablation.txt):
  // 256 x 128 tiles halve the W bytes per flop and a third stage keeps two K tiles in flight: +7..13 % (r2_gemm_cfg_probe.txt)
  if constexpr (NP == 1) return launch_split_cfg<256, 128, 8, 1, 3, NP, 2>(d, s);
  if constexpr (NP == 2) return launch_split_cfg<128, 128, 4, 1, 2, NP, 2>(d, s);   // held to 2 wavefronts per SIMD
  return launch_split_cfg<128, 128, 2, 2, 2, NP, 2>(d, s);
}

// W [rows][K] fp32 -> W2h [rows][K/32][2][32] fp16 (k permuted as above) of w * 2^e_row, e_row chosen so that
// the row's max |w| lands in [2^14, 2^15); col_scale[row] = 2^-e_row (exact).  One wavefront per row.
__global__ __launch_bounds__(256) void split_weights_h2_kernel(const float* __restrict__ W, int64_t rows, int K,
                                                               int64_t ldw, u16* __restrict__ W2, float* __restrict__ col_scale) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float m = 0.f;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(W[r * ldw + k]));
  m = wave_max(m);
  float sc, inv;
  h2_scale(m, sc, inv);
  if (lane == 0) col_scale[r] = inv;
  for (int k = lane; k < K; k += 64) {
    const float x = W[r * ldw + k] * sc;
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    const int kk = k & 31;
    const int pos = 8 * ((kk & 15) >> 2) + (kk & 3) + 4 * (kk >> 4);
    u16* o = W2 + r * 2 * K + (int64_t)(k >> 5) * 64 + pos;
    o[0] = __builtin_bit_cast(u16, h);
    o[32] = __builtin_bit_cast(u16, l);
  }
}

}  // namespace

int launch_gemm_split(const dzn_gemm_desc& d, hipStream_t s) {
  if ((d.K & 31) || (d.kc & 31) || d.ldw != d.K) return DZN_E_INVALID;
  if (d.A2 && prec_is_h2(d.precision) && d.a_amax && !d.a2_amax) return DZN_E_INVALID;   // one scale from BOTH bounds
  // fp16 two-term path: needs the fp16 planes + their row scales, the producer-tracked |max| of A, and weights
  // that do not move with z (col_scale is indexed by the output column alone)
  const bool no_h2 = gemm_no_h2();
  // DZN_PREC_F16 with the MX planes: fp16 hi*hi + fp8 cross terms (gemm_mx.hip); without them the single-term fp16 kernel
  if (d.precision == DZN_PREC_F16 && d.Wmx && d.col_scale_mx && d.a_amax && !d.w_z0 && !d.w_z1 && !no_h2)
    return launch_gemm_mx(d, s);
  if (prec_is_h2(d.precision) && d.W2h && d.col_scale && d.a_amax && !d.w_z0 && !d.w_z1 && !no_h2) {
    if (d.precision == DZN_PREC_F16) return launch_gemm_split_np<1>(d, s);
    return launch_gemm_split_np<2>(d, s);
  }
  if (!d.W3) return DZN_E_INVALID;
  return launch_gemm_split_np<3>(d, s);
}

int launch_split_weights_h2(const float* W, int64_t rows, int K, int64_t ldw, void* W2, float* col_scale, hipStream_t s) {
  if (rows <= 0) return DZN_OK;
  if (K <= 0 || (K & 31)) return DZN_E_INVALID;
  hipLaunchKernelGGL(split_weights_h2_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, s, W, rows, K, ldw,
                     static_cast<u16*>(W2), col_scale);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_op_split_weights_h2(const float* W, int64_t rows, int32_t K, int64_t ldw, void* W2, float* col_scale,
                                       void* stream) {
  if (!W || !W2 || !col_scale) return DZN_E_INVALID;
  return launch_split_weights_h2(W, rows, K, ldw, W2, col_scale, reinterpret_cast<hipStream_t>(stream));
}

int launch_split_weights(const float* W, int64_t rows, int K, int64_t ldw, void* W3, hipStream_t s) {
  if (rows <= 0) return DZN_OK;
  if (K <= 0 || (K & 31)) return DZN_E_INVALID;
  int64_t g = cdiv64(rows * K, 256);
  g = g > 8192 ? 8192 : g;
  hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)g), dim3(256), 0, s, W, rows, K, ldw,
                     static_cast<u16*>(W3));
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_op_split_weights(const float* W, int64_t rows, int32_t K, int64_t ldw, void* W3, void* stream) {
  if (!W || !W3) return DZN_E_INVALID;
  return launch_split_weights(W, rows, K, ldw, W3, reinterpret_cast<hipStream_t>(stream));
}
