/*
 * dzn_ops.h — kernel-level entry points of libdzn_hip.so.
 *
 * These expose the individual gfx950 kernels the engine is built from, on raw device
 * pointers, so that tests/ can check each kernel against a plain fp32 reference of the
 * same op (torch on the host side) and bench.py can time a kernel in isolation.  They
 * are not part of the drop-in surface (that is dzn.h); they have no reference-side
 * counterpart other than the torch op named in each comment.
 *
 * All functions enqueue on `stream` and return 0 / negative DZN_E_* (see dzn.h).
 */
#ifndef DZN_OPS_H_
#define DZN_OPS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* activations applied to (acc + bias) */
#define DZN_ACT_NONE 0
#define DZN_ACT_GELU 1  /* exact erf GELU, torch.nn.functional.gelu */
#define DZN_ACT_SWISH 2 /* x * sigmoid(x) */
#define DZN_ACT_RELU 3

/*
 * Generic MFMA contraction  C[m,n] = epilogue( sum_k A(m,k) * W[n,k] ).
 *
 *   A(m,k)   = A[ zA + rowbase(m) + (k / kc) * ldk + (k % kc) ]
 *   rowbase  = a_rowoff ? a_rowoff[m] : m * lda            (element offsets)
 *   W[n,k]   = W[ zW + n * ldw + k ]                        (torch Linear / packed conv layout)
 *   acc      = rstd[m] * (acc - mean[m] * ln_colsum[n])      if ln_stats  (LayerNorm folded into the weights)
 *   v        = act(acc + bias[zB + n]) * alpha
 *   v       += R[ zC + crow(m) + n ]        if R            crow = c_rowoff ? c_rowoff[m] : m*ldc
 *   v        = max(v, 0)                    if post_relu
 *   C[ zC + crow(m) + n ] = v
 *   WS[ m*ldws + n ] (+)= ws_w * v          if WS   ('=' when ws_init)
 *
 * The two-level K addressing (kc, ldk) turns 1-D / 2-D convolutions over channels-last
 * activations into this same contraction without an im2col copy.  grid.z batches:
 * z -> (z0 = z / zdiv, z1 = z % zdiv), zA = z0*a_z0 + z1*a_z1 etc.
 * Requirements: K % 32 == 0, kc % 32 == 0, all strides/offsets multiples of 4 elements.
 */
typedef struct dzn_gemm_desc {
  const float* A;
  const float* W;        /* fp32 weights */
  float* C;
  const float* bias;
  const float* R;
  float* WS;
  const int32_t* a_rowoff;
  const int32_t* c_rowoff;
  int32_t M, N, K;
  int64_t lda;
  int32_t kc;
  int64_t ldk;
  int32_t ldw;
  int64_t ldc;
  int64_t ldws;
  int32_t act;
  float alpha;
  int32_t post_relu;
  float ws_w;
  int32_t ws_init;
  int32_t nz, zdiv;
  int64_t a_z0, a_z1, w_z0, w_z1, c_z0, c_z1, b_z0, b_z1;
  int32_t precision;     /* DZN_PREC_* (DZN_PREC_BF16 is reserved: DZN_E_INVALID) */
  double alg_flops;      /* algorithmic flops of this launch for profiling (0 -> 2*M*N*K*nz) */
  /* DZN_PREC_F32_SPLIT only: the weights pre-split into three bf16 planes by dzn_op_split_weights
   * (same z / row offsets as W, times 3); NULL, K % 32 or kc % 32 != 0 -> fp32 MFMA kernel */
  const void* W3;
  /* DZN_PREC_F32_SPLIT only: A is ALREADY split — `A` points at plane 0 of three bf16 planes a_plane
   * elements apart, written by the producer in the weight planes' k order (csrc/gemm_split_pre.hip) */
  int32_t a_split3;
  int64_t a_plane;
  /* LayerNorm folded into this contraction (pre-norm sites: y = LN(x) feeds only linears): A is the RAW row x,
   * W already carries gamma (W' = W diag(gamma)), bias carries W beta, and the epilogue finishes the norm with the
   * per-row statistics: acc = rstd[m] * (acc - mean[m] * ln_colsum[n]), ln_colsum[n] = sum_k W'[n,k].
   * ln_stats = f32 [M][2] (mean, rstd) written by dzn_op_row_stats / the fused gate kernel; NULL = plain. */
  const float* ln_stats;
  const float* ln_colsum;
  /* DZN_PREC_F32_H2 ("f32h"): two-term fp16 split, three products (csrc/gemm_split.hip, NP = 2).
   * W2h = planes from dzn_op_split_weights_h2 ([rows][K/32][2][32] fp16 of w * 2^e_row), col_scale[n] = 2^-e_row,
   * a_amax = device array of per-unit bounds >= max |A| (tracked by the producer of A through c_amax, or dzn_op_amax).  Any of them
   * NULL -> the bf16 three-term kernel (W3).  c_amax (any mode): atomically max'ed with |C| as stored. */
  const void* W2h;
  const float* col_scale;
  const float* a_amax;
  float* c_amax;
  /* a_amax / c_amax are ARRAYS with one |max| per scale unit, so that a window's result does not depend on the rest
   * of the batch: unit of row m = m / amax_unit when amax_unit > 0 (rows of one window), else the z0 batch index. */
  int32_t amax_unit;
  /* LayerNorm statistics of the OUTPUT rows for a following folded LayerNorm: the epilogue leaves per-row partial
   * (sum, sum of squares) in stat_partial (f32 [M][P][2] scratch, P = column tiles x wavefront columns <= 32) and the
   * launcher reduces them to stat_final f32 [M][2] = (mean, rstd) over stat_C columns (plain z == 1 launches only). */
  float* stat_partial;
  float* stat_final;
  int32_t stat_C;
  float stat_eps;
  /* z-batched launches over a SUBSET of the z0 indices that is chosen ON THE DEVICE (the embedding trunk skips windows
   * without an active speaker without a host round trip): the launch still has nz grid rows; grid row y works on
   * z0 = z_list[y / zdiv] when y / zdiv < z_count[0] and exits otherwise.  NULL = every z0. */
  const int32_t* z_count;
  const int32_t* z_list;
  /* DZN_PREC_F16 (r5): the reduced-precision contraction of csrc/gemm_mx.hip — fp16 hi*hi plus the two cross terms in fp8 on the
   * block-scaled matrix instruction.  Wmx = planes from dzn_op_split_weights_mx ([rows][K/32][128 B]: fp16 hi | fp8 hi, fp8 lo of
   * w * 2^e_row), col_scale_mx[n] = 2^-e_row; needs a_amax like the fp16 two-term form.  Either NULL -> the single-term fp16
   * kernel on the leading plane of W2h (r2-r4's DZN_PREC_F16 arithmetic, kept for the positional conv and the ResNet trunk). */
  const void* Wmx;
  const float* col_scale_mx;
  /* number of entries of the a_amax / c_amax arrays (0 = not stated): only read by CHECKED builds (csrc/checked.h), which
   * assert that every scale-unit index stays inside them */
  int32_t amax_count;
  /* (r6) attention operands written by the q/k/v contraction itself (csrc/attention_planes.hip; reference arithmetic
   * W2V/components.py:453-486): the columns n >= kv_col0 of C = [q | k | v] x heads x 64 — the K and V slots — are NOT stored to C
   * as fp32; every (row, 64-column head slot) is scaled by the exact power of two that puts its own |max| into [2^14, 2^15) and
   * stored as the two fp16 terms of the f32h split: kv_planes = fp16 [2][rows][kv_ld] (plane p at p * kv_plane_stride elements,
   * row-major, kv_ld = N - kv_col0), kv_scale = f32 [rows][kv_ld / 64] = the INVERSE scale of the slot.  The attention kernel then
   * stages ready tiles (no split, no 7-fold re-split per query tile) and un-scales per key.  NULL = plain fp32 store.  Needs the
   * 16x16-block f32h / f32s contraction kernels, kv_col0 % 64 == 0 and N % 64 == 0 (refused otherwise). */
  void* kv_planes;
  int64_t kv_plane_stride;
  float* kv_scale;
  int32_t kv_ld;
  int32_t kv_col0;
  /* A SECOND A segment (the 1x1 stride-2 shortcut of a ResNet down-sampling block folded into conv2: one sum over a longer K,
   * no shortcut image in memory).  K columns k < k1 address A as above; columns k1 <= k < k1 + k2 read
   *   A2[ z0 * a2_z0 + a2_rowoff[m] + (k - k1) ]
   * and the columns from k1 + k2 up to K (the zero-padded weight columns of the last tile) are NEVER read or multiplied, so a
   * non-finite neighbour of the k2 run cannot reach the sum.  a2_amax = the per-unit |max| array of the second source, indexed
   * like a_amax: the fp16 forms scale BOTH segments by the power of two of max(a_amax[u], a2_amax[u]).  NULL A2 = one segment.
   * Requirements (DZN_E_INVALID otherwise): k1 % 64 == 0, k1 >= 128, k2 % 32 == 0, k1 + k2 <= K < k1 + k2 + 64, a2_rowoff set,
   * a2_amax set where a_amax is used; taken by the fp32 LDS-DMA kernel (csrc/gemm.hip) and by csrc/gemm_split.hip — the MX
   * (csrc/gemm_mx.hip) and pre-split (a_split3) forms refuse it. */
  const float* A2;
  const int32_t* a2_rowoff;
  const float* a2_amax;
  int64_t a2_z0;
  int32_t k1, k2;
} dzn_gemm_desc;

/* (r4) One BasicBlock of the 32-channel ResNet stage in one kernel (csrc/resblock_fused.hip):
 * out = relu(conv2(relu(conv1(in) + b1)) + b2 + in) over zero-bordered NHWC fp32 images [B][Hs+2][Ws+2][32]; W1 / W2 = fp16
 * two-term planes of the folded [32][288] weights (dzn_op_split_weights_h2), cs = their inverse row scales, amax_in f32 [B]
 * = per-image max |in|, l1max1 = max_oc sum_k |W1[oc][k]|, bmax1 = max_oc |b1[oc]| (bound of the intermediate). */
int dzn_op_resblock32_fused(const float* in, float* out, const void* W1, const float* cs1, const float* b1, const void* W2,
                            const float* cs2, const float* b2, const float* amax_in, float l1max1, float bmax1, int32_t B,
                            int32_t Hs, int32_t Ws, void* stream);

/* (r4) The same block with producer / consumer wavefronts (csrc/resblock_ws.hip), C = 32 or 64 planes: images
 * [B][Hs+2][Ws+2][C], W = planes of the folded [C][9 C] weights with k = (dh*3 + dw) * C + ci. */
int dzn_op_resblock_ws(const float* in, float* out, const void* W1, const float* cs1, const float* b1, const void* W2,
                       const float* cs2, const float* b2, const float* amax_in, float l1max1, float bmax1, int32_t B,
                       int32_t Hs, int32_t Ws, int32_t C, void* stream);

/* test knob: terms per operand the two entry points above run with — 2 (default, DZN_PREC_F32_H2) or 1 (the DZN_PREC_F16 form:
 * leading fp16 term only, plane 0 of the same weight buffers) */
int dzn_op_set_resblock_np(int32_t np);
/* (r5) test switch of the attention kernels (csrc/attention_split.hip): 1 = the wavefronts of a partial last query tile that own no
 * query compute scores / softmax / P.V as r2-r4 did; the stored bits are the same. */
int dzn_op_set_attention_noskip(int32_t on);

int dzn_op_gemm(const dzn_gemm_desc* d, void* stream);

/* Exact 3-way bf16 split of fp32 weights for DZN_PREC_F32_SPLIT (csrc/gemm_split.hip):
 * W fp32 [rows][K] (row stride ldw, K % 32 == 0) -> W3 bf16 [rows][K/32][3][32] (3*rows*K u16). */
int dzn_op_split_weights(const float* W, int64_t rows, int32_t K, int64_t ldw, void* W3, void* stream);

/* fp16 two-term split of fp32 weights for DZN_PREC_F32_H2: W2h fp16 [rows][K/32][2][32] (2*rows*K u16) of
 * W * 2^e_row with max|row| in [2^14, 2^15), col_scale f32 [rows] = 2^-e_row. */
int dzn_op_split_weights_h2(const float* W, int64_t rows, int32_t K, int64_t ldw, void* W2h, float* col_scale,
                            void* stream);

/* planes of the reduced-precision contraction (DZN_PREC_F16, csrc/gemm_mx.hip): Wmx = 128 bytes per (row, 32 k) = 4 * rows * K
 * bytes — fp16 of w * 2^e_row (64 B, fragment order) then four 16-B slots [fp8 e4m3 of w * 2^e_row x 8 | fp8 of the fp16
 * remainder * 2^11 x 8]; max|row| * 2^e_row in [2^7, 2^8); col_scale f32 [rows] = 2^-e_row. */
int dzn_op_split_weights_mx(const float* W, int64_t rows, int32_t K, int64_t ldw, void* Wmx, float* col_scale,
                            void* stream);
/* CHECKED builds only (python -m diarizen_amd.build --checked, csrc/checked.h): device-side bounds assertions in the hand-
 * scheduled kernels (LDS stage / fragment offsets, tracker indices, tile ranges).  out4 (may be NULL) = {failed checks since the
 * last reset, id of the first, its workgroup, its detail value}; reset != 0 clears the counters.  Returns the number of failed
 * checks (0 = clean), DZN_E_STATE in a release build. */
int dzn_checked_status(uint32_t* out4, int32_t reset);

/* tests / tuning: force one tile shape of csrc/gemm_mx.hip ("128x128", "128x64", "256x128"; "auto" / "" / NULL = the shape
 * rule) for the calls that follow.  Same effect as the DZN_GEMM_MX_CFG environment variable, which is read on first use. */
int dzn_op_set_gemm_mx_cfg(const char* cfg);

/* tests / tuning: force one tile shape, by name, for the calls that follow; "auto" / "" / NULL = the shape heuristic.  Same effect
 * as the DZN_GEMM_CFG environment variable, which is read on first use.  One name reaches all three non-MX families, and a
 * family that does not know it keeps its heuristic:
 *   csrc/gemm.hip            "128x32", "256x32", "256x64", "128x64", "64x64", "128x128"
 *   csrc/gemm_split.hip      "128x64", "128x80", "128x32", "128x128" (f32s) / "128x128w4" (f32h, f16), "256x128w8s3" (f16)
 *   csrc/gemm_split_pre.hip  "256x128", "128x128", "128x64"
 * While a name is set, launches that ask for K / V planes (kv_planes) are refused: only the automatic tiles write them. */
int dzn_op_set_gemm_cfg(const char* cfg);

/* amax[0] = max(amax[0], max |x[0..n)|) — the |max| tracker of a tensor whose producer has no fused tracker */
int dzn_op_amax(const float* x, int64_t n, float* amax, void* stream);

/* fp32 rows [rows, D] (D % 32 == 0) -> three bf16 planes [rows, D], plane_stride elements apart, channels of
 * every 32-block in fragment order: the pre-split A operand (dzn_gemm_desc.a_split3) */
int dzn_op_split_rows(const float* x, void* planes, int64_t plane_stride, int64_t rows, int32_t D, void* stream);

/* x fp32 [B, L, G * cg] -> the two fp16 planes (DZN_PREC_F32_H2) of its zero-padded copy [B, Lp, D = G * cgp], rows shifted
 * by `pad`, plane_stride elements apart, channels cg .. cgp - 1 of a group zero (cgp % 32 == 0), every 32-block in fragment order.
 * Window b is scaled by the power of two of amax[b] (>= max |x[b]|), which is copied to snapshot[b] for the consumer's a_amax. */
int dzn_op_pad_rows_split2(const float* x, void* planes, int64_t plane_stride, int32_t B, int32_t L, int32_t Lp, int32_t pad,
                           int32_t D, const float* amax, float* snapshot, int32_t cg, int32_t cgp, void* stream);

/* The positional convolution on RESIDENT plane rows (csrc/posconv_resident.hip): C[b L + t, g cg + n] = epilogue(sum over taps j
 * and the group's 64 plane channels of planes[b, t + j, g 64 + c] * W[g cg + n, j 64 + c]).  d is the descriptor the generic
 * pre-split contraction (dzn_op_gemm, a_split3 == 2) takes for the same conv: A = the planes of dzn_op_pad_rows_split2 with
 * Lp = L + taps and cgp == 64, a_plane, ldk = D, a_z1 = kc = 64, M = B * L, N = cg <= 64, K = ldw = taps * 64, nz = zdiv = G, w_z1,
 * c_z1, b_z1, W2h / col_scale, a_amax = the snapshot, amax_unit = L, precision = DZN_PREC_F32_H2; a_rowoff is not read.  C is
 * bit-identical to dzn_op_gemm's.  DZN_E_INVALID for any other descriptor and for a shape whose rows do not fit LDS
 * (dzn_op_posconv_resident_fits == 0: B windows of L rows, `taps` taps). */
int dzn_op_posconv_resident(const dzn_gemm_desc* d, int32_t B, int32_t L, int32_t taps, void* stream);
int dzn_op_posconv_resident_fits(int32_t B, int32_t L, int32_t taps);

/* 3x3 stride-1 convolution 32 -> 32 channels over zero-bordered fp32 NHWC images [B][Hs+2][Ws+2][32]
 * (first ResNet34 stage, wespeaker/resnet.py:139-144 with BatchNorm folded into W / bias) in the fp32-split
 * arithmetic: W3 = dzn_op_split_weights of W [32][(dh*3+dw)*32 + ci]; out = post_relu?max(0,·):(·) of
 * (relu?max(0,·):(·))(conv + bias) + R.  Only interior pixels are written (borders stay zero). */
int dzn_op_conv3x3_c32(const float* in, const void* W3, const float* bias, const float* R, float* out,
                       int32_t B, int32_t Hs, int32_t Ws, int32_t relu, int32_t post_relu, void* stream);

/* the same convolution in the fp16 two-term arithmetic (DZN_PREC_F32_H2): W2h / col_scale = dzn_op_split_weights_h2 of
 * W [32][288], amax_in = f32 [B] per-image |max| of `in` */
int dzn_op_conv3x3_c32_h2(const float* in, const void* W3, const void* W2h, const float* col_scale, const float* amax_in,
                          const float* bias, const float* R, float* out, int32_t B, int32_t Hs, int32_t Ws,
                          int32_t relu, int32_t post_relu, void* stream);

/* The three image kernels in the launch form the engine uses (tests: nothing fixed, nothing filled, nothing allocated).
 *   amax_out  f32 [B] or NULL: amax_out[b] = max(amax_out[b], max |out[b]|) for every image the launch works on
 *   z_count / z_list  int32 [1] / int32 [<= B] or NULL: the launch works on images z_list[0 .. z_count[0]) only; one of the two
 *                     without the other means all B images
 *   np        (blocks) terms per operand: 2 (DZN_PREC_F32_H2) or 1 (DZN_PREC_F16); anything else is DZN_E_INVALID
 * conv: W2h, col_scale and amax_in all given -> the fp16 two-term form (W3 may be NULL), none of them -> the bf16 three-term
 * form (W3 required); some but not all -> DZN_E_INVALID.  dzn_op_resblock_ws_ex: C other than 32 / 64 is DZN_E_INVALID. */
int dzn_op_conv3x3_c32_ex(const float* in, const void* W3, const void* W2h, const float* col_scale, const float* amax_in,
                          const float* bias, const float* R, float* out, int32_t B, int32_t Hs, int32_t Ws, int32_t relu,
                          int32_t post_relu, float* amax_out, const int32_t* z_count, const int32_t* z_list, void* stream);
int dzn_op_resblock32_fused_ex(const float* in, float* out, const void* W1, const float* cs1, const float* b1, const void* W2,
                               const float* cs2, const float* b2, const float* amax_in, float* amax_out, float l1max1,
                               float bmax1, int32_t B, int32_t Hs, int32_t Ws, int32_t np, const int32_t* z_count,
                               const int32_t* z_list, void* stream);
int dzn_op_resblock_ws_ex(const float* in, float* out, const void* W1, const float* cs1, const float* b1, const void* W2,
                          const float* cs2, const float* b2, const float* amax_in, float* amax_out, float l1max1, float bmax1,
                          int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t np, const int32_t* z_count,
                          const int32_t* z_list, void* stream);

/* y[r,:] = LayerNorm(x[r,:C]) * gamma + beta (eps), optional fused erf-GELU; row strides
 * ldx / ldy; columns [C, Cpad) of y are written as zero.  torch F.layer_norm. */
int dzn_op_layernorm(const float* x, int64_t ldx, float* y, int64_t ldy, const float* gamma,
                     const float* beta, int64_t rows, int32_t C, int32_t Cpad, float eps,
                     int32_t gelu, void* stream);

/* stats[r] = (mean, 1/sqrt(var + eps)) of x[r, :C] (biased variance, two passes over registers): the row
 * statistics of torch F.layer_norm for a LayerNorm that is folded into the consuming contraction. */
int dzn_op_row_stats(const float* x, int64_t ldx, int64_t rows, int32_t C, float eps, float* stats, void* stream);

/* gate_a_1[row, H] of WavLM's gated relative position bias (W2V/components.py:702-710):
 * y f32 [rows, ldy] (attention input, Htot*64 wide), Wg [8,64], bg [8], cst [Htot]. */
int dzn_op_gate(const float* y, int64_t ldy, const float* Wg, const float* bg, const float* cst,
                float* gate, int64_t rows, int32_t Htot, void* stream);

/*
 * Fused multi-head attention with optional WavLM gated relative-position bias
 * (W2V/components.py:453-486, 690-725; conformer.py:47-71).
 *   qkv   f32 [B*L, ldqkv]: q at col 0, k at col h*64, v at col 2*h*64 (head-major, 64 each)
 *   out   f32 [B*L, ldo]  : head j at cols j*64..
 *   gate  f32 [B*L, Htot] or NULL: gate_a_1 per (row, ORIGINAL head)
 *   table f32 [Htot, 2L-1] or NULL: rel-pos bias by (key - query + L - 1)
 *   head_idx i32 [h] device: original head index of kept head j
 */
/* pre-norm fusion of the two above: one pass over the raw residual rows x [rows, Htot*64] writes the LayerNorm
 * statistics stats [rows][2] (for a contraction with folded gamma / beta) and gate[rows, Htot] evaluated on
 * LayerNorm(x) * gamma + beta. */
int dzn_op_gate_stats(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* Wg,
                      const float* bg, const float* cst, float* gate, float* stats, int64_t rows, int32_t Htot,
                      float eps, void* stream);
/* (mean, rstd) [rows][2] of rows of C elements from P (sum, sum of squares) pairs per row, f32 [rows][P][2], as a contraction
 * epilogue leaves them (dzn_gemm_desc.stat_partial): the kernel dzn_op_gemm runs when stat_final is set */
int dzn_op_stats_finalize(const float* partial, int64_t rows, int32_t P, int32_t C, float eps, float* stats, void* stream);
/* the same for rows whose LayerNorm partial sums a producing contraction has left (dzn_gemm_desc.stat_partial, P <= 32 pairs
 * of (sum, sum of squares) per row, over C = Htot*64 channels): stats [rows][2] = what the finalize kernel gives from the same
 * partials, bit for bit, and gate[row, H] for the h heads H listed in head_idx (i32 [h], device) — only their 64 channels of x
 * are read; the other columns of gate are left as they are.  DZN_E_INVALID unless 1 <= h <= Htot <= 16 and 1 <= P <= 32. */
int dzn_op_gate_heads(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* Wg,
                      const float* bg, const float* cst, const int32_t* head_idx, int32_t h, const float* stat_partial,
                      int32_t P, int32_t C, float eps, float* gate, float* stats, int64_t rows, int32_t Htot,
                      void* stream);

/* the same attention in the fp16 two-term arithmetic (DZN_PREC_F32_H2): amax = f32 [B], |max| of each window's qkv */
int dzn_op_attention_h2(const float* qkv, float* out, const float* gate, const float* table, const int32_t* head_idx,
                        int32_t B, int32_t L, int32_t h, int32_t Htot, int32_t ldqkv, int32_t ldo, float scale,
                        const float* amax, void* stream);

/* (r6) the attention on PRE-SPLIT K / V (csrc/attention_planes.hip): packs the K and V slots of a plain fp32 qkv = [B L][3 h 64]
 * into fp16 two-term planes with one power-of-two scale per (row, head slot) — exactly what the q/k/v contraction's epilogue
 * writes (dzn_gemm_desc.kv_planes) — and runs the kernel the engine runs.  planes / kvs: caller's scratch, fp16 [2][B L + 64][2 h 64]
 * and f32 [B L + 64][2 h], zero-filled by the caller. */
int dzn_op_attention_planes(const float* qkv, float* out, const float* gate, const float* table, const int32_t* head_idx,
                            int32_t B, int32_t L, int32_t h, int32_t Htot, int32_t ldqkv, int32_t ldo, float scale,
                            const float* amax, void* planes, float* kvs, void* stream);

/* test / A-B switch of the planes kernel: 16-query blocks per wavefront — 1 (default: 64 queries per workgroup, three workgroups
 * per CU) or 2 (128 queries per workgroup: every staged tile and LDS fragment read serves twice the matrix work; measured 4 % SLOWER,
 * profiles/r6_attention_planes_ab.txt) */
int dzn_op_set_attention_qb(int32_t query_blocks_per_wavefront);
/* ... and whether the next K / V tile is requested before the current one is computed (default 1) */
int dzn_op_set_attention_prefetch(int32_t on);

int dzn_op_attention(const float* qkv, float* out, const float* gate, const float* table,
                     const int32_t* head_idx, int32_t B, int32_t L, int32_t h,
                     int32_t Htot, int32_t ldqkv, int32_t ldo, float scale,
                     int32_t precision, void* stream);

/*
 * The small (non-contraction) kernels, one entry point per launcher: tests/test_small_kernels_gpu.py holds each against a float64
 * reference of the operation named here.  Outputs and row strides are the caller's, so a test can surround every buffer with a
 * pattern band.  Arguments a launcher cannot serve return DZN_E_INVALID before anything is enqueued.
 */
/* csrc/conformer.hip: out[b,t,c] = swish(bias[c] + sum_j w[c,j] g[b, t + j - (ks-1)/2, c]), g = u[.., c] * sigmoid(u[.., A + c]),
 * zero outside [0, L) of the window's own rows (GLU -> depthwise Conv1d -> folded BatchNorm -> Swish); u [B L, ldu >= 2 A],
 * out [B L, ldo >= A], w [A, ks], ks in {7, 15, 31}. */
int dzn_op_glu_dwconv(const float* u, int64_t ldu, const float* w, const float* bias, float* out, int64_t ldo, int32_t B,
                      int32_t L, int32_t A, int32_t ks, void* stream);
/* logits = z[r, :A] W^T + bias (W [NC, A], NC <= 16); logp [rows, NC] = log_softmax, multilabel u8 [rows, S] =
 * mapping[argmax] (first maximum; mapping u8 [NC, S], S <= 64), soft [rows, S] = exp(logp) @ mapping; each output may be NULL. */
int dzn_op_classify(const float* z, int64_t ldz, const float* W, const float* bias, const uint8_t* mapping, int64_t rows,
                    int32_t A, int32_t NC, int32_t S, float* logp, uint8_t* multilabel, float* soft, void* stream);
/* The front end of a segmentation forward (tests/test_frontend_kernels_gpu.py).
 * HOST: lnq110[0 .. 10) = mean over the C0 channels of the taps w [C0, k] (k <= 10), lnq110[10 + 10 e + j] = F[e][j] with
 * F^T F = the covariance over channels of the taps; entries of taps >= k are zero.  The statistics conv0 takes from a frame's
 * samples x: mean_c y = wbar . x, var_c y = |F x|^2. */
int dzn_op_conv0_lnq(const float* w, int32_t C0, int32_t k, float* lnq110);
/* csrc/frontend.hip: out[b, f, c] = sum_t w[c, t] x[b, f s + t], x = (wave - stats[b, 0]) * stats[b, 1] (stats NULL: x = wave);
 * layer_norm = 1: then LayerNorm over the C0 channels of the frame (gamma, beta) and erf-GELU, the statistics from lnq (above)
 * or, lnq NULL, from the frame's outputs.  wave [B, N], out [B, T0, Cp] with columns [C0, Cp) zero; Cp % 4 == 0, k <= 10, s <= 8,
 * C0 <= 512, (T0 - 1) s + k <= N. */
int dzn_op_conv0(const float* wave, int32_t B, int32_t N, const float* stats, const float* w, const float* gamma, const float* beta,
                 int32_t C0, int32_t Cp, int32_t k, int32_t s, int32_t T0, int32_t layer_norm, float eps, float* out,
                 const float* lnq, void* stream);
/* csrc/frontend_fused.hip: the values of dzn_op_split_weights_h2(W [rows, K] contiguous) in fragment-major order
 * [K/32][rows/16][2][16][32] fp16, col_scale f32 [rows]; rows % 16 == 0, K % 32 == 0. */
int dzn_op_split_weights_h2_frag(const float* W, int32_t rows, int32_t K, void* W2h, float* col_scale, void* stream);
/* conv0 (k 10, s 5, LayerNorm from lnq, GELU) -> conv1 (k 3, s 2) in one kernel, fp16 two-term arithmetic:
 * out[b, t, n] = sum_{j < 3, c < C0} W[n, j C0 + c] a[b, 2 t + j, c], a = dzn_op_conv0's output; gamma1 / beta1 non-NULL: then LayerNorm
 * over the C1 real channels and GELU, and amax1 (f32 [B] or NULL) is max'ed with |out| (raw output: amax1 is not touched).
 * W2h / col_scale = dzn_op_split_weights_h2_frag of W [N1p, 3 C0] with zero rows n >= C1; act_bound >= max |a| (static:
 * sqrt(C0) max|gamma0| + max|beta0|).  out [B, T1, N1p].  C0 % 64 == 0, C0 >= 128, N1p == 160, 80 < C1 <= 160 with gamma1,
 * (T0 - 1) 5 + 10 <= N, T0 >= 3, T1 <= (T0 - 3) / 2 + 1; wstats, gamma1, beta1, amax1 may be NULL. */
int dzn_op_conv01_fused(const float* wave, int32_t B, int32_t N, const float* wstats, const float* w0, const float* gamma0,
                        const float* beta0, const float* lnq, int32_t C0, int32_t T0, int32_t T1, const void* W2h,
                        const float* col_scale, int32_t N1p, float act_bound, float eps, float* out, const float* gamma1,
                        const float* beta1, int32_t C1, float* amax1, void* stream);
/* csrc/frontend.hip: y[b,t,c] = gelu((x[b,t,c] - mean[b,c]) * rstd[b,c] * gamma[c] + beta[c]) with the statistics over the T
 * rows of window b (GroupNorm(C, C), biased variance), columns [C, Cp) of y zero; x, y [B T, ld] (y may be x), Cp % 4 == 0,
 * ld % 4 == 0, Cp <= 1024; stats = scratch of dzn_op_gn_stats_floats() floats; amax f32 [B] or NULL: max'ed with |y|. */
int dzn_op_groupnorm_gelu(const float* x, float* y, int32_t B, int32_t T, int32_t C, int32_t Cp, int64_t ld, const float* gamma,
                          const float* beta, float eps, float* stats, float* amax, void* stream);
int64_t dzn_op_gn_stats_floats(int32_t B, int32_t T, int32_t C, int32_t Cp);
/* xpad[b, t + pad, :] = x[b, t, :], every other row of xpad [B, Lp, D] zero; D % 4 == 0 */
int dzn_op_pad_rows(const float* x, float* xpad, int32_t B, int32_t L, int32_t Lp, int32_t pad, int32_t D, void* stream);
/* ws = (init ? 0 : ws) + w * x over n floats (n % 4 == 0) */
int dzn_op_ws_accum(const float* x, float* ws, float w, int32_t init, int64_t n, void* stream);
/* ws = ((0 + w[0] x[0]) + w[1] x[1]) + ...: xs = HOST array of `count` device pointers, weights = HOST array (count <= 40) */
int dzn_op_ws_sum(const float* const* xs, const float* weights, int32_t count, float* ws, int64_t n, void* stream);
/* x[r, c] *= scale[c] for c < C; columns [C, ld) untouched */
int dzn_op_col_scale(float* x, int64_t rows, int32_t C, int64_t ld, const float* scale, void* stream);
/* csrc/norm.hip: dzn_op_layernorm + post (f32 [C] or NULL: multiplied in after the GELU) + amax (f32 [units] or NULL: entry
 * row / amax_unit, or entry 0 when amax_unit == 0, is max'ed with |y|); gamma and beta may each be NULL. */
int dzn_op_layernorm_t(const float* x, int64_t ldx, float* y, int64_t ldy, const float* gamma, const float* beta,
                       const float* post, int64_t rows, int32_t C, int32_t Cpad, float eps, int32_t gelu, float* amax,
                       int64_t amax_unit, void* stream);
/* stats[b] = (mean, 1 / sqrt(var + eps)) of the N samples of window b (biased variance) */
int dzn_op_wave_stats(const float* w, int32_t B, int32_t N, float eps, float* stats, void* stream);
/* csrc/embed.hip: Kaldi framing.  frames[b T + t, :flen] = window * pre-emphasis(x - mean(x)), x = 2^15 * wave[b stride + t fshift
 * + (0 .. flen)], previous sample of the first = itself; columns [flen, Kp) zero; flen <= 512. */
int dzn_op_frame_prep(const float* wave, int32_t B, int64_t stride, int32_t T, int32_t flen, int32_t fshift, int32_t Kp,
                      const float* window, float preemph, float* frames, void* stream);
/* pw[r, f] = |spec[r, f] + i spec[r, nb + f]|^2, spec [rows, 2 nb] */
int dzn_op_power(const float* spec, int64_t rows, int32_t nb, float* pw, void* stream);
/* mel [B, T, NB] in place: log(max(mel, eps)) minus its mean over the T frames of the window */
int dzn_op_log_cmn(float* mel, int32_t B, int32_t T, int32_t NB, float eps, void* stream);
/* the same out of place from a shared frame grid: window b's frame t = row b q + t of mel; fb [B, T, NB] */
int dzn_op_log_cmn_gather(const float* mel, int32_t q, float* fb, int32_t B, int32_t T, int32_t NB, float eps, void* stream);
/* img[b, 1 + h, 1 + t, c] = relu(bias[c] + sum_{dh,dw} w[c, 3 dh + dw] fb[b, t + dw - 1, h + dh - 1]) (zero outside), fb [B, T, NB],
 * img [B, NB + 2, T + 2, C] whose border is not written; C % 4 == 0 and 256 % (C / 4) == 0; amax f32 [B] or NULL;
 * (z_count, z_list): both or neither, the images to compute, chosen on the device (dzn_gemm_desc.z_list) */
int dzn_op_stem_conv(const float* fb, int32_t B, int32_t T, int32_t NB, int32_t C, const float* w, const float* bias, float* img,
                     float* amax, const int32_t* z_count, const int32_t* z_list, void* stream);
/* weighted mean / std over the W interior columns of img [B, H + 2, W + 2, C] for each of S masks [B, S, L], the mask
 * interpolated to W frames as F.interpolate(mode="nearest") does; stats [B, S, 2 C H], feature c H + h; active i32 [B] or
 * NULL: windows with active[b] == 0 get zeros and their image is not read.  S W floats of LDS: above 64 KiB is refused. */
int dzn_op_stats_pool(const float* img, int32_t B, int32_t H, int32_t W, int32_t C, const float* masks, int32_t S, int32_t L,
                      float* stats, const int32_t* active, void* stream);
/* flag[b] = any of the per_window mask values of window b is non-zero */
int dzn_op_window_active(const float* masks, int32_t B, int32_t per_window, int32_t* flag, void* stream);
/* list[0 .. count[0]) = the b with flag[b] != 0, ascending; totals (i64 [2] or NULL) += (B, B - count[0]) */
int dzn_op_compact_active(const int32_t* flag, int32_t B, int32_t* count, int32_t* list, int64_t* totals, void* stream);

/*
 * In-situ kernel timing (HIP events on the launch stream).  Enable, run forwards, then collect:
 * one entry per kernel class with the number of launches, the summed event time and the summed
 * ALGORITHMIC flops / HBM bytes declared by the launch sites (un-padded reference shapes).
 */
typedef struct dzn_prof_entry {
  char name[64];
  int64_t launches;
  double ms;
  double flops;
  double bytes;
} dzn_prof_entry;
int dzn_profile_enable(int32_t on);
int dzn_profile_collect(dzn_prof_entry* out, int32_t cap, int32_t* n);
/* pre-create n_events HIP events (two per launch at most) so that a timed region never allocates one */
int dzn_profile_reserve(int32_t n_events);

/* host-side relative-position bucket of WavLM (W2V/components.py:629-666), exposed for tests */
int dzn_op_relpos_bucket(int32_t rel, int32_t num_buckets, int32_t max_distance);

#ifdef __cplusplus
}
#endif
#endif
