// posconv_resident.hip — the positional convolution (W2V/components.py:366-380) as a Toeplitz-RESIDENT contraction, for the
// fp16 two-term planes of pad_rows_split2_kernel (DZN_PREC_F32_H2, NP = 2) and 64 plane channels per group.
//
// gemm_split_pre.hip runs the conv as a generic contraction: every K tile (tap j, 32-channel block) fetches a new A tile by
// LDS-DMA, and that tile is the previous tap's tile shifted by one padded row.  Here a workgroup owns one (group, 256 flat
// output rows) item, brings the padded plane rows its taps touch into LDS ONCE, and walks the taps reading A fragments from
// the resident rows at a row offset of +j.  Only the W planes stream through the stage ring.
//
// Tile geometry.  Flat tiles of BM = 256 rows over B * L, as the generic path (a tile may straddle windows;
// no per-window padding), BN = 64 = the group, 8 wavefronts of 32 x 64 (MI = 2, NI = 4, the wavefront tile of the 128 x 64
// generic kernel: 12 ds_read_b128 per 24 MFMAs).  Output row m = b L + t reads padded rows prow(m) + j, prow(m) = m + (m / L) Kc,
// so the rows of a tile span at most  span = BM - 1 + Kc (1 + nb)  padded rows, nb = min((L + BM - 2) / L, B - 1) window
// boundaries inside a tile (posconv_span below).  L = 399, Kc = 128: 511 rows -> 512 x 256 B = 128 KB resident + 3 x 8 KB of W
// stages = 152 KB of the 160 KB: ONE workgroup of 8 wavefronts (two per SIMD) per CU, pinned by __launch_bounds__(512) and the
// LDS size; 148 VGPRs, no AGPRs, no scratch (hipcc -Rpass-analysis=kernel-resource-usage).  Four wavefronts of 64 x 64 (one per
// SIMD, 224 + 88 registers) measured 9.7 ms per launch at the model's shape against 8.9 ms for this form and 11.7 ms for the
// generic kernel.  A shape whose span does not fit is not taken (posconv_resident_fits): the generic kernel
// keeps it.
//
// LDS image of the resident rows: per (plane, 32-channel block) an array [span16 rows][64 B], 16-byte chunk c of LDS row r
// stored at slot c ^ ((r >> 1) & 3).  Bank arithmetic (ds_read_b128: bank = (addr / 4) % 64, i.e. a 256-B bank row of sixteen
// 16-B slots; slot index of (r, c) = 4 (r & 3) + (c ^ key(r)); lanes conflict inside the four 16-lane groups {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, ...): a group reads 16 CONSECUTIVE rows R .. R + 15 (R = any offset: the tap moves it), rows R + {0-3,
// 12-15} with chunk a and rows R + {4-11} with chunk a ^ 1.  Rows of one class r & 3 are r0, r0 + 4, r0 + 8, r0 + 12 and carry
// chunks a, a ^ 1, a ^ 1, a; key(r) = (r >> 1) & 3 = bit 1 of the class + 2 x bit 2 of r, and bit 2 alternates along r0 + 4 k:
// keys u, u ^ 2, u, u ^ 2 -> slots a ^ u, a ^ u ^ 3, a ^ u ^ 1, a ^ u ^ 2: four distinct slots per class, sixteen in all,
// conflict free at EVERY R.  The key of the aligned tiles, g((r >> 2) & 3) with g = (0, 2, 3, 1) (pswz, gemm_split_pre.hip), is
// NOT: along r0 + 4 k its keys are g(q), g(q + 1), g(q + 2), g(q + 3), and q = 1 gives slots a ^ 2, a ^ 1 ^ 3 = a ^ 2: two-way
// for every second q.  It is conflict free only at R % 16 == 0, which is all the aligned tiles need; the W stages keep it.
// tests/test_posconv_resident_math.py walks both statements over every offset.
//
// Same bits as gemm_split_pre_kernel<.., NP = 2>: per accumulator the products run taps ascending, then the group's two
// 32-blocks, then lo*hi, hi*lo, hi*hi; 16-row blocks start at multiples of 16 flat rows in both; the epilogue is the shared one.
#include "common.h"
#include "gemm_epilogue.h"
#include "gemm_launch.h"
#include "split.h"

namespace {

constexpr int PR_BM = 256, PR_BN = 64, PR_NW = 8, PR_S = 3;
constexpr int PR_LDS_MAX = 160 * 1024;

__device__ __forceinline__ int pswz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }   // W stages (aligned rows)
__device__ __forceinline__ int rswz(int row) { return (row >> 1) & 3; }                          // resident rows (any offset)

template <int N>
__device__ __forceinline__ void wait_vm_lgkm0() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4));
}

// L rows per window, Kc taps, prows = B (L + Kc) padded rows in the planes, span16 = resident rows (a multiple of 16,
// >= posconv_span).  d as the engine builds it for the generic path (planes in d.A, d.ldk = plane row width, z1 = group).
template <int BM, int NW, int S>
__global__ __launch_bounds__(NW * 64) void posconv_resident_kernel(const dzn_gemm_desc d, const int L, const int Kc, const int prows,
                                                               const int span16) {
  constexpr int BN = PR_BN, BK = 32, NP = 2;
  constexpr int TM = BM / NW, TN = BN;
  constexpr int MI = TM / 16, NI = TN / 16, MH = MI / 2;
  constexpr int WPLANE = BN * 64, WBUF = NP * WPLANE;     // one W stage: 64 rows x 64 B x 2 planes
  constexpr int WPIECES = NP * BN / 16;                   // 1-KB pieces (plane, 16 rows) of a W stage: piece = 4 plane + rows / 16
  constexpr int LPT = WPIECES / NW;                        // LDS-DMA instructions per wavefront and stage
  static_assert(BN == 64 && WPIECES % NW == 0 && LPT >= 1, "whole W pieces per wavefront");
  static_assert(MI % 2 == 0, "two row halves per wavefront tile");
  static_assert(S >= 2 && (S - 1) * LPT < 64, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave;
  int tm, tn, z0, z1;
  if (!gemm_tile(d, 1, tm, tn, z0, z1)) return;
  const u16* __restrict__ A2p = reinterpret_cast<const u16*>(d.A) + z1 * d.a_z1;
  const u16* __restrict__ W2 = reinterpret_cast<const u16*>(d.W2h) + NP * (z1 * d.w_z1);
  const int IMG = span16 * 64;                             // bytes of one (plane, block) image
  unsigned char* const sWring = smem + 4 * IMG;

  const int m0 = tm * BM;
  const int pfirst = m0 + (m0 / L) * Kc;                   // padded row of LDS row 0
  const int lr = lane & 15, lq = lane >> 4;
  float row_inv[MI];
  int arow[MI];                                            // LDS row of this lane's output row at tap 0
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    int m = m0 + wm * TM + i * 16 + lr;
    m = m < d.M ? m : d.M - 1;
    const int b = m / L;
    float unused;
    h2_scale(d.a_amax[b], unused, row_inv[i]);
    arow[i] = m + b * Kc - pfirst;
  }
  const int64_t cz = z1 * d.c_z1;
  const int64_t bz = z1 * d.b_z1;

  // ---- resident rows: 16-row pieces of 1 KB per wavefront instruction, piece q = NW round + wave; thread -> (row 16 q +
  // lane / 4, physical slot lane % 4), logical chunk = slot ^ rswz(row); rows past the planes' end repeat the last one
  // (never read by a stored output row) ----
  {
    const int npieces = span16 >> 4;
    for (int q = wave; q < npieces; q += NW) {
      const int r = q * 16 + (lane >> 2);
      int p = pfirst + r;
      p = p < prows ? p : prows - 1;
      const u16* src = A2p + (int64_t)p * d.ldk + (((lane & 3) ^ rswz(r)) << 3);
      unsigned char* dst = smem + q * 1024;
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pl * d.a_plane + h * 32),
                                           (__attribute__((address_space(3))) void*)(dst + (pl * 2 + h) * IMG), 16, 0, 0);
    }
  }

  // ---- W stages: thread -> (row 16 (wave % 4) + lane / 4, slot lane % 4), the image of gemm_split_pre.hip ----
  // wavefront w fills pieces w, w + NW, ..: piece c = (plane c / 4, rows 16 (c % 4) ..)
  const int pr0 = (wave & 3) * 16 + (lane >> 2);
  const u16* wptr;
  {
    const int n = pr0 < d.N ? pr0 : d.N - 1;
    wptr = W2 + (int64_t)n * NP * d.ldw + (((lane & 3) ^ pswz(pr0)) << 3);
  }
  int ik = 0;
  auto issue = [&](int stage) {
    unsigned char* sW = sWring + stage * WBUF + wave * 1024;
#pragma unroll
    for (int c = 0; c < LPT; ++c) {
      const int p = (wave + c * NW) >> 2;                  // wave-uniform plane of this piece
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wptr + NP * ik + p * 32),
                                       (__attribute__((address_space(3))) void*)(sW + c * NW * 1024), 16, 0, 0);
    }
    ik += BK;
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int woff[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int row = j * 16 + lr;
    woff[j] = row * 64 + ((lq ^ pswz(row)) << 4);
  }
  auto read_w = [&](int stage, u32x4 (&wf)[NI][NP]) {
    const unsigned char* base = sWring + stage * WBUF;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int p = 0; p < NP; ++p) wf[j][p] = *reinterpret_cast<const u32x4*>(base + p * WPLANE + woff[j]);
  };
  // K tile kt = (tap kt / 2, 32-block kt % 2): the resident rows at offset + tap
  auto read_a = [&](int kt, u32x4 (&af)[MI][NP]) {
    const int tap = kt >> 1;
    const unsigned char* base = smem + (kt & 1) * IMG;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int r = arow[i] + tap;
      const int off = r * 64 + ((lq ^ rswz(r)) << 4);
#pragma unroll
      for (int p = 0; p < NP; ++p) af[i][p] = *reinterpret_cast<const u32x4*>(base + p * 2 * IMG + off);
    }
  };
  // products of one 16-row block, smallest terms first (same order as gemm_split_pre.hip)
  auto mma = [&](int i, const u32x4 (&wf)[NI][NP], const u32x4 (&a)[NP]) {
    constexpr int PW[3] = {1, 0, 0}, PA[3] = {0, 1, 0};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] = mfma_np<NP>(wf[j][PW[t]], a[PA[t]], acc[i][j]);
  };

  const int nk = 2 * Kc;
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s < nk) issue(s);
  if (nk >= S) wait_vm_lgkm0<(S - 1) * LPT>();     // loads retire in order: the resident rows and stage 0 have landed
  else wait_vm_lgkm0<0>();
  __builtin_amdgcn_s_barrier();
  u32x4 wfa[NI][NP], wfb[NI][NP], af[MI][NP];
  read_w(0, wfa);
  read_a(0, af);
  int stage = 0;
  auto step = [&](int kt, const u32x4 (&wc)[NI][NP], u32x4 (&wn_)[NI][NP]) {
    const bool more = kt + 1 < nk;
#pragma unroll
    for (int i = 0; i < MH; ++i) mma(i, wc, af[i]);
    u32x4 a2[MI - MH][NP];
#pragma unroll
    for (int i = MH; i < MI; ++i)
#pragma unroll
      for (int p = 0; p < NP; ++p) a2[i - MH][p] = af[i][p];
    const int nstage = stage + 1 == S ? 0 : stage + 1;
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      if (kt + S <= nk) wait_vm_lgkm0<(S - 2) * LPT>();
      else wait_vm_lgkm0<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + S < nk) issue(stage);
      read_w(nstage, wn_);
      read_a(kt + 1, af);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = MH; i < MI; ++i) mma(i, wc, a2[i - MH]);
    stage = nstage;
  };
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, wfa, wfb);
    step(kt + 1, wfb, wfa);                        // nk = 2 Kc is even
  }
  // column vectors of the epilogue in LDS (the resident rows are dead by now)
  __syncthreads();
  gemm_epilogue<BM, BN, TM, TN, MI, NI, true>(d, acc, tm, 0, wm, 0, lr, lq, cz, bz, z0, row_inv, d.col_scale + bz,
                                              reinterpret_cast<float*>(smem) + wm * 3 * TN);
}

// padded rows a BM-row tile's taps touch, at most (see the header)
int posconv_span(int B, int L, int Kc, int BM) {
  int nb = (L + BM - 2) / L;
  nb = nb < B - 1 ? nb : B - 1;
  return BM - 1 + Kc * (1 + nb);
}

size_t posconv_lds(int span16) { return (size_t)span16 * 256 + (size_t)PR_S * 2 * PR_BN * 64; }

}  // namespace

// Does the resident kernel take a positional conv of B windows of L rows with Kc taps?  (Only the LDS span can say no.)
bool posconv_resident_fits(int B, int L, int Kc) {
  if (B <= 0 || L <= 0 || Kc <= 0) return false;
  const int span16 = round_up(posconv_span(B, L, Kc, PR_BM), 16);
  return posconv_lds(span16) <= (size_t)PR_LDS_MAX;
}

// d: the descriptor of the generic path (engine.cpp seg_project): planes in A (a_split3 == 2, a_plane), ldk = plane row width,
// a_z1 = 64 channels per group, M = B L flat rows, N <= 64, K = Kc * 64, nz = zdiv = groups, amax_unit = L.  a_rowoff is not read.
int launch_posconv_resident(const dzn_gemm_desc& din, int B, int L, int Kc, hipStream_t s) {
  dzn_gemm_desc d = din;
  if (d.M <= 0 || d.N <= 0) return DZN_OK;
  if (d.alpha == 0.f) d.alpha = 1.f;
  if (d.nz <= 0) d.nz = 1;
  const bool ok = d.A && d.C && d.a_split3 == 2 && d.a_plane > 0 && d.precision == DZN_PREC_F32_H2 && d.W2h && d.col_scale &&
                  d.a_amax && B > 0 && L > 0 && Kc > 0 && (int64_t)B * L == d.M && d.N <= PR_BN && d.a_z1 == 64 && d.kc == 64 &&
                  d.K == Kc * 64 && d.ldw == d.K && d.ldk >= 64 && !(d.ldk & 7) && !(d.a_plane & 7) && d.amax_unit == L &&
                  d.zdiv == d.nz && !d.z_list && !d.A2 && !d.stat_partial && !d.kv_planes && !d.ln_stats && !d.c_rowoff &&
                  (int64_t)B * (L + Kc) * d.ldk < (int64_t)1 << 31 && posconv_resident_fits(B, L, Kc);
  if (!ok) return DZN_E_INVALID;
  const int span16 = round_up(posconv_span(B, L, Kc, PR_BM), 16);
  const size_t lds = posconv_lds(span16);
  const int tilesM = (d.M + PR_BM - 1) / PR_BM;
  int pid = -1;
  if (prof_enabled()) {
    // algorithmic bytes: the planes once, W once per tile, C and the residual
    const double nz = d.nz;
    double bytes = (double)B * (L + Kc) * 64.0 * nz * 4.0;               // two fp16 planes
    bytes += (double)tilesM * nz * d.N * (double)d.K * 4.0;               // two fp16 planes of W per (tile, group)
    bytes += (double)d.M * d.N * 4.0 * nz * (d.R ? 2.0 : 1.0);
    const double fl = d.alg_flops > 0 ? d.alg_flops * nz : 2.0 * d.M * d.N * (double)d.K * nz;
    pid = prof_begin(s, "posconv_f32h", fl, bytes);
  }
  constexpr auto KERN = posconv_resident_kernel<PR_BM, PR_NW, PR_S>;
  static unsigned long long attr_mask = 0;
  if (first_use_on_device(attr_mask))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, PR_LDS_MAX);
  hipLaunchKernelGGL(KERN, dim3(tilesM, d.nz, 1), dim3(PR_NW * 64), lds, s, d, L, Kc, B * (L + Kc), span16);
  prof_end(pid, s);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_op_posconv_resident(const dzn_gemm_desc* d, int32_t B, int32_t L, int32_t taps, void* stream) {
  if (!d) return DZN_E_INVALID;
  return launch_posconv_resident(*d, B, L, taps, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dzn_op_posconv_resident_fits(int32_t B, int32_t L, int32_t taps) { return posconv_resident_fits(B, L, taps) ? 1 : 0; }

// the producer of the planes, for tests of the kernel alone (engines call the launcher): x fp32 [B, L, G * cg] -> two fp16
// planes of the zero-padded copy [B, Lp, D = G * cgp] scaled per window by amax[b], which is copied to snapshot[b]
extern "C" int dzn_op_pad_rows_split2(const float* x, void* planes, int64_t plane_stride, int32_t B, int32_t L, int32_t Lp,
                                      int32_t pad, int32_t D, const float* amax, float* snapshot, int32_t cg, int32_t cgp,
                                      void* stream) {
  if (!x || !planes || B <= 0 || L <= 0 || Lp < L + pad || pad < 0 || plane_stride < (int64_t)B * Lp * D) return DZN_E_INVALID;
  return launch_pad_rows_split2(x, planes, plane_stride, B, L, Lp, pad, D, amax, snapshot, reinterpret_cast<hipStream_t>(stream),
                                cg, cgp);
}
