// engine.cpp — the C ABI of include/dzn.h: weight ingest (fold + pack + pad), workspace, and the
// host-side orchestration of the gfx950 kernels for the two device stages of the DiariZen
// pipeline: the WavLM + Conformer segmentation forward and the ResNet34 embedding forward.
//
// Data layout in HBM (all activations fp32, channels-last, feature dims zero-padded to
// multiples of 32 so every contraction has K % 32 == 0 and 16-byte aligned rows):
//   conv stack   [B, T_i, Cp_i]         — conv i reads conv i-1 as overlapping rows (lda = s*Cp)
//   encoder      x, y, ws [B*L, D]      — residual stream, LN output, layer-weighted sum
//   attention    qkv [B*L, 3*h*64], gate [B*L, H], bias table [H, 2L-1]
//   ResNet       zero-bordered NHWC images [B, H+2, W+2, C]; 3x3 convs address them through
//                per-geometry row-offset tables (no im2col)
// Weights are folded on the host at finalize: weight-norm of the positional conv
// (W2V/components.py:344), eval BatchNorm of the Conformer conv module (conformer.py:205) and of
// every ResNet conv (resnet.py:139-144), q/k/v concatenation, conv weights re-ordered to
// [out][tap][in].
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <array>
#include <vector>

#include "common.h"

#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      throw EngineError(e_ == hipErrorOutOfMemory ? DZN_E_NOMEM : DZN_E_HIP,             \
                        std::string(#x) + ": " + hipGetErrorString(e_));                 \
    }                                                                                    \
  } while (0)

namespace {

struct EngineError : std::runtime_error {
  int code;
  EngineError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct HostT {
  std::vector<float> v;
  std::vector<int64_t> shape;
};

struct Lin {       // y = x W^T + b with W [N, K] (rows zero-padded to Np, cols to Kp)
  float* W = nullptr;
  u16* W3 = nullptr;   // exact 3-way bf16 split planes (DZN_PREC_F32_SPLIT), gemm_split.hip layout
  float* b = nullptr;
  u16* W2h = nullptr;  // two-term fp16 planes of W * 2^e_row (DZN_PREC_F32_H2) ...
  float* wsc = nullptr;   // ... and 2^-e_row per output row (dzn_gemm_desc.col_scale)
  float* csum = nullptr;  // LayerNorm folded into W (make_lin_ln): column sums of W diag(gamma), dzn_gemm_desc.ln_colsum
  unsigned char* Wmx = nullptr;   // DZN_PREC_F16: planes of the reduced-precision contraction (gemm_mx.hip: fp16 hi | fp8 hi, fp8 lo) ...
  float* wsc_mx = nullptr;        // ... and their inverse row scales (dzn_gemm_desc.col_scale_mx)
  int N = 0, K = 0;    // padded sizes
  int Nt = 0, Kt = 0;  // reference (un-padded) sizes, for algorithmic flop accounting
};

struct LNp {
  float* g = nullptr;
  float* b = nullptr;
  int C = 0;
};

// A LayerNorm that feeds a linear, loaded by norm_lin() and run by norm_lin_desc(): the one place that decides, and the one
// that acts on, whether the norm is folded into the weights.  ln.C == 0: no norm in front (post-norm encoder layers).
struct NormLin {
  LNp ln;
  Lin lin;
  bool folded = false;   // gamma / beta are inside lin.W / lin.b and lin.csum is set (make_lin_ln): the contraction reads RAW rows
};

struct EncLayer {
  bool attn = false, ffn = false;
  bool pre_norm = false;   // layer_norm_first: ln1 / ln2 stand in front of qkv / f1 (and live in them); else they follow the sub-blocks
  int h = 0, F = 0, Fp = 0;
  LNp ln1, ln2;
  NormLin qkv, f1;
  Lin out, f2;
  float *Wg = nullptr, *bg = nullptr, *cst = nullptr;
  int32_t* head_idx = nullptr;
  // the rows this layer's first LayerNorm reads come with their statistics: the previous layer's FFN-down epilogue leaves
  // the partial sums (decided at finalize: Switches::epilogue_stats, pre-norm, both norms folded, a predecessor with an FFN)
  bool stats_in = false;
};

struct ConfLayer {
  NormLin ffn1_w1, ffn2_w1, qkv, pw1;   // each with the ln_norm of its sub-block
  Lin ffn1_w2, ffn2_w2, o, pw2;
  LNp out_ln;
  float *dw = nullptr, *dwb = nullptr;
};

struct ResConv {
  Lin l;
  int cin = 0, cout = 0, ksz = 3, stride = 1;
  int k2 = 0;   // > 0: conv2 of a down-sampling block with the 1x1 shortcut folded in — k2 more K columns from the previous stage's image
  float l1max = 0.f, bmax = 0.f;   // max_oc sum_k |W[oc][k]| and max_oc |shift[oc]| of the folded conv: |out| <= amax(in) l1max + bmax
  // decided at finalize (finalize_emb), from the arithmetic mode, the switches and the weight planes that exist
  bool c32 = false;     // 3x3 stride 1 over 32 planes in a split mode: the first stage's dedicated kernel (conv_split.hip)
  bool keep2 = false;   // DZN_PREC_F16: this contraction keeps two fp16 terms (bit CLS_RESNET of Switches::f16_keep2)
};
// A BasicBlock and the kernels it runs as (decided at finalize, finalize_emb; acted on by emb_block):
//   PER_CONV     stride 1: conv1 and conv2 as a launch each
//   FUSED32      stride 1, 32 planes, two-term fp16 modes: both convolutions in one kernel (resblock_fused.hip)
//   WS           stride 1, 32 or 64 planes, two-term fp16 modes: the producer / consumer form (resblock_ws.hip)
//   DOWN         first block of stages 2-4: stride-2 conv1, the 1x1 shortcut as its own launch (sc), conv2 adds it
//   DOWN_FOLDED  ... the 1x1 shortcut is c2.k2 more K columns of conv2 (make_resconv_shortcut)
struct ResBlock {
  enum Form { PER_CONV, FUSED32, WS, DOWN, DOWN_FOLDED };
  ResConv c1, c2, sc;
  Form form = PER_CONV;
  int np = 2;   // fp16 terms per operand in the FUSED32 / WS kernels
};
// One stage of the ResNet trunk over an fbank image of given size: what a launch over its images needs (stage_geometry; the
// tables by emb_set_geometry).
struct EmbStage {
  int s, Hs, Ws, Cc;       // images of Hs x Ws pixels, Cc planes innermost, stored with a one-pixel zero border
  int64_t img, interior;   // elements of one image with its border; offset of pixel (0, 0) behind the border
  int M;                   // Hs * Ws: rows of a contraction over one image
  int32_t *tab1, *tab2;    // device, row y * Ws + x -> offset of its 3x3 patch here / of pixel (2y, 2x) in the previous stage
};

std::string last_create_error;

// contraction classes: the value is the bit index of the DZN_F16_KEEP2 / DZN_F16_MX masks (DZN_PREC_F16: classes whose bit
// is set keep two fp16 terms per operand / run the fp8 cross terms).  0-13 are the segmentation model's, 14 the ResNet trunk.
enum F16Class { CLS_CONV, CLS_FEATPROJ, CLS_POSCONV, CLS_QKV, CLS_OUT, CLS_FFN1, CLS_FFN2, CLS_PROJ, CLS_CONF_W1, CLS_CONF_W2,
                CLS_CONF_QKV, CLS_CONF_OUT, CLS_CONF_PW1, CLS_CONF_PW2, CLS_RESNET };
// what a failed launch of a segmentation class is called in the error message
const char* const F16_CLASSES[CLS_RESNET] = {"conv gemm", "feature projection", "pos conv", "qkv", "out_proj", "ffn1", "ffn2",
                                             "proj", "conf ffn w1", "conf ffn w2", "conf qkv", "conf out", "conf pw1", "conf pw2"};

// Every DZN_* environment switch the engine reads.  All of them are read once, by read_switches() at dzn_create: a switch
// belongs to the handle that was created under it.
struct Switches {
  bool fold_ln = true;          // fp32 engine modes: LayerNorms that feed only linears are folded (make_lin_ln)
  bool conv0_quad_stats = true;
  bool fuse_conv01 = true;
  bool conv01_ln = true;
  // (r4) pre-norm encoders: every layer writes its output rows into ITS OWN buffer (xl + layer * rows * D) and the
  // layer-weighted sum (model_wavlm_conformer.py:236,253-254) is ONE pass over those buffers after the last layer, instead of
  // a read-modify-write of `ws` in every FFN-output epilogue: 25 reads + 1 write of [rows, D] where there were 25 reads and
  // 25 writes.  Off: the fused read-modify-write (also taken by post-norm encoders and when there is not enough free memory).
  bool ws_defer = true;
  bool att_planes = true;
  bool epilogue_stats = true;
  bool emb_skip = true;
  bool fuse_resblock = true;    // (r4) stride-1 BasicBlocks in the two-term fp16 modes: both convolutions in one kernel
  bool fuse_shortcut = true;    // off: the shortcut of a down-sampling block stays its own launch
  bool posconv_resident = true; // off: the positional conv stays on the generic pre-split contraction
  int resblock_ws = 2;          // bit mask: 1 = 32-plane blocks, 2 = 64-plane blocks on the producer / consumer form
  // DZN_PREC_F16 (reduced precision): which contraction classes keep two fp16 terms (F16Class bit mask; bit 14 = the
  // ResNet stages 2-4), and whether LayerNorm-folded single-term contractions subtract the row mean BEFORE rounding
  // defaults from profiles/r4_f16_sensitivity.json (64 non-degenerate windows vs the f32h engine): the error of the
  // single-term mode is NOT localised — no one class brings max |dlogp| under SURVEY 8d's 5e-2, only two terms everywhere
  // (= f32h) does; the conv stack alone carries ~70 % of the error variance for 4 % of the flops, so it keeps two terms
  // (0.247 -> 0.133, flips 0.52 % -> 0.33 %); centring the LayerNorm-folded split changes nothing (0.228 vs 0.247: the
  // error is plain operand rounding, not the mean * colsum cancellation) and stays off.
  // (r5) bit 14 governs the whole trunk: the stride-2 / shortcut / stage 3-4 contractions (gemm_split.hip NP = 1)
  // AND the fused stride-1 BasicBlocks of stages 1-2 (resblock_fused.hip / resblock_ws.hip, which have a single-term form
  // since r5; in r4 they were two-term whatever the bit said).
  // (r5) with the cross terms in fp8 everywhere else, the Conformer head (bits 8-13, 8 % of the segmentation flops) keeps two
  // fp16 terms as well: max |dlogp| does not move (1.01e-2 vs 1.03e-2) but the decisions next to the classifier do — DER of the
  // mode's RTTM against the fp32 RTTM on the 30 s fixture 0.05 % (one 20 ms frame) instead of 0.17 % (three), inside SURVEY 8d's
  // 0.1 abs; device step 1872 -> 1856 audio-s/s on one box (profiles/r5_reduced_mode_keep2_probe.txt)
  unsigned f16_keep2 = 0x3f01;
  // (r5) DZN_PREC_F16: the classes whose bit is set run fp16 hi*hi + the two cross terms in fp8 (gemm_mx.hip) — every linear
  // contraction of the segmentation model: the class sweep of profiles/r4_reduced_mode_emulation.txt shows that any one of them
  // at a single fp16 term costs 0.04-0.21 of max |dlogp| against SURVEY 8d's 5e-2, only the positional conv (bit 2) can stay at
  // one term.  Bit 0 (the conv stack) keeps two fp16 terms (f16_keep2).  0 = r4's single-term mode.
  unsigned f16_mx = 0x3ffa;
  bool debug_taps = false;
};

Switches read_switches() {
  Switches s;
  s.fold_ln = !getenv("DZN_NO_LN_FOLD");                    // =1: every LayerNorm runs stand-alone, in the reference's order
  s.conv0_quad_stats = !getenv("DZN_CONV0_WAVE_STATS");      // =1: conv0's LayerNorm statistics from its outputs, not the quadratic form
  s.fuse_conv01 = !getenv("DZN_NO_CONV01_FUSION");          // =1: conv0 and conv1 as separate kernels (f32h)
  s.conv01_ln = !getenv("DZN_CONV01_NO_LN");                // =1: the fused conv0 -> conv1 kernel leaves conv1's LayerNorm + GELU to the row pass
  s.ws_defer = !getenv("DZN_NO_WS_DEFER");                  // =1: layer-weighted sum as a read-modify-write in every FFN-output epilogue
  s.att_planes = !getenv("DZN_NO_ATT_PLANES");              // =1: fp32 K / V and the in-kernel split of attention_split.hip (f32h)
  s.epilogue_stats = !getenv("DZN_NO_EPILOGUE_STATS");      // =1: every LayerNorm's statistics by a pass over its rows (gate_stats / row_stats), none from a producing epilogue
  s.emb_skip = !getenv("DZN_EMB_NO_SKIP");                  // =1: windows without an active speaker go through the trunk too
  s.fuse_resblock = !getenv("DZN_NO_RESBLOCK_FUSION");      // =1: the per-conv kernels for the stride-1 BasicBlocks
  s.fuse_shortcut = !getenv("DZN_NO_SHORTCUT_FUSION");      // =1: the 1x1 shortcut of a down-sampling block as its own launch
  s.posconv_resident = !getenv("DZN_NO_POSCONV_RESIDENT");  // =1: the positional conv stays on the generic pre-split contraction (f32h)
  if (const char* e = getenv("DZN_RESBLOCK_WS")) s.resblock_ws = atoi(e);                      // which fused blocks take the producer / consumer form
  if (const char* e = getenv("DZN_F16_KEEP2")) s.f16_keep2 = (unsigned)strtoul(e, nullptr, 0); // reduced mode: classes with two fp16 terms
  if (const char* e = getenv("DZN_F16_MX")) s.f16_mx = (unsigned)strtoul(e, nullptr, 0);       // reduced mode: classes with fp8 cross terms
  const char* dbg = getenv("DZN_DEBUG_TAPS");               // =1: every stage's output is copied to the host for dzn_debug_fetch
  s.debug_taps = dbg && dbg[0] == '1';
  return s;
}

}  // namespace

struct dzn_handle {
  dzn_config cfg{};
  int device = 0;  // HIP device current at dzn_create: every entry point makes it current again
  std::string err;
  std::map<std::string, HostT> sd;
  std::set<std::string> used;
  int ignored = 0;
  bool finalized = false;
  Switches sw;
  std::vector<void*> allocs;
  int64_t bytes = 0;
  std::map<std::string, std::vector<float>> taps;

  // ---- segmentation: geometry ----
  int nconv = 0;
  int C[DZN_MAX_CONV]{}, Cp[DZN_MAX_CONV]{};
  int D = 0, H = 0, A = 0, Fh = 0;
  // ---- segmentation: weights ----
  float* conv0_w = nullptr;
  float* conv0_lnq = nullptr;    // [10 + 100]: mean and covariance factor over channels of conv0's taps (frontend.hip)
  u16* conv1_W2f = nullptr;      // conv1's fp16 planes in fragment-major order [K/32][Cp1/16][2][16][32] and
  float* conv1_wscf = nullptr;   // their row scales [Cp1]: the fused conv0 -> conv1 kernel (frontend_fused.hip); null = not fused
  LNp conv_ln[DZN_MAX_CONV];
  Lin conv[DZN_MAX_CONV];
  float* dummy_w = nullptr;
  LNp enc_ln;
  NormLin fp;
  Lin posconv;
  int pos_rowD = 0;               // row width the row-offset table of the positional conv was built for
  int pos_cgp = 0;                // channels per positional-conv group in the pre-split planes (cg rounded up to 32)
  bool posconv_resident = false;  // the positional conv takes posconv_resident.hip where a call's span fits LDS (fixed at create)
  std::vector<EncLayer> layers;
  std::vector<float> rel_embed;  // [num_buckets, H] host
  std::vector<float> wsum_w;
  Lin proj;
  LNp lnorm;
  std::vector<ConfLayer> conf;
  float *cls_w = nullptr, *cls_b = nullptr;
  uint8_t* mapping = nullptr;
  // rel-pos table cache
  int table_L = -1;
  int pos_L = -1;               // geometry baked into pos_rowoff
  int32_t* pos_rowoff = nullptr;  // row m = b*L + t of the positional conv -> element offset into xpad
  u16* xpad3 = nullptr;           // f32s mode: the padded copy as three bf16 planes (split once, read by 128 taps)
  int64_t xpad3_plane = 0;
  float* table = nullptr;
  // ---- segmentation: workspace ----
  int maxT[DZN_MAX_CONV]{};
  int maxL = 0;
  float *stats = nullptr, *gn_stats = nullptr, *bufA = nullptr, *bufB = nullptr;
  float *x = nullptr, *xpad = nullptr, *y = nullptr, *ws = nullptr, *qkv = nullptr, *ao = nullptr,
        *gate = nullptr, *mid = nullptr;
  float *hz = nullptr, *ht = nullptr, *hmid = nullptr, *hv = nullptr;
  // (r6) K / V of the encoder's attention as pre-split fp16 planes + per-(row, head slot) inverse scales, written by the q/k/v
  // contraction's epilogue (csrc/attention_planes.hip); nullptr = fp32 K / V and the in-kernel split of attention_split.hip
  void* kvp = nullptr;
  float* kvs = nullptr;
  int64_t kvp_rows = 0;
  int kvp_ldmax = 0;
  float* xl = nullptr;      // per-layer output buffers of the deferred layer-weighted sum (Switches::ws_defer); nullptr: not deferred
  int64_t xl_elems = 0;     // size xl would have (0: not applicable to this model / switched off)
  float* spart = nullptr;   // [max_batch * maxL][32][2] per-row partial sums left by a producing epilogue (stat_partial)
  float* rstat = nullptr;   // [max_batch * maxL][2] (mean, rstd) of the LayerNorm folded into the next contraction
  // |max| trackers of activation tensors (DZN_PREC_F32_H2), ONE PER WINDOW of the batch (slot * max_batch + b): written
  // by the producer's epilogue / LayerNorm, read by the consuming contraction to scale its fp16 split
  // (gemm_split.hip).  Per window, so a window's result is independent of the batch it runs in.  Zeroed per forward.
  enum { AM_CONVA, AM_CONVB, AM_X, AM_XPAD, AM_Y, AM_MID, AM_QKV, AM_HZ, AM_HMID, AM_IMG0, AM_COUNT = AM_IMG0 + 12 };
  float conv0_bound = 0.f;  // sqrt(C0) max|gamma| + max|beta| >= |GELU(LN(conv0))|: static |max| of conv0's output
  float* amax = nullptr;

  // ---- embedding ----
  bool has_emb = false;
  float *hamming = nullptr;
  Lin dft, mel, seg1;
  float *stem_w = nullptr, *stem_b = nullptr;
  std::vector<std::vector<ResBlock>> stages;
  int emb_T = -1;  // geometry currently baked into tables / borders
  int maxTf = 0;
  int sC[4]{};
  float* sbuf[4][3]{};
  int64_t sbuf_elems[4]{};  // allocation per image at the largest geometry
  struct EmbGeom {          // per fbank-frame-count T: row-offset tables stay resident, so alternating window
    EmbStage stage[4]{};    // lengths (full windows / a ragged tail) neither re-upload nor synchronise
  };
  std::map<int, EmbGeom> geoms;
  const EmbStage* stage = nullptr;   // the four stages at the CURRENT geometry (emb_T; owned by geoms)
  float *frames = nullptr, *spec = nullptr, *pw = nullptr, *fb = nullptr, *pool = nullptr;
  // fbank rows per pass of frame_prep -> DFT -> power -> mel (frames / spec / pw hold that many rows: the frame grid of
  // max_batch windows a tenth of a window apart) and the mel energies of a shared frame grid, [<= max_batch * maxTf, NB]
  int64_t fb_rows = 0;
  float* melg = nullptr;
  // trunk skip for windows without any active speaker (r3; r4: decided on the device): flag per window, the ascending
  // list of active windows + its length, running totals (windows seen, windows skipped) for dzn_embed_skip_stats
  int *win_flag = nullptr, *win_idx = nullptr, *win_cnt = nullptr;
  long long* emb_totals = nullptr;
  long long emb_dense_windows = 0;   // windows that went through the trunk on the dense path (no subset: nothing to skip)
  bool mx_pack = false;   // make_lin also packs the MX planes (set while the segmentation weights are finalized)
};

namespace {

using H = dzn_handle;

// ------------------------------------------------------------------ device memory helpers
template <typename T>
T* dalloc(H* h, int64_t n, bool zero = true) {
  if (n <= 0) n = 1;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, n * sizeof(T)));
  h->allocs.push_back(p);
  h->bytes += n * (int64_t)sizeof(T);
  if (zero) HIPCHK(hipMemset(p, 0, n * sizeof(T)));
  return reinterpret_cast<T*>(p);
}

float* upload(H* h, const std::vector<float>& v) {
  float* p = dalloc<float>(h, (int64_t)v.size(), false);
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return p;
}

int pad32(int v) { return round_up(v, 32); }

const HostT& need(H* h, const std::string& key) {
  auto it = h->sd.find(key);
  if (it == h->sd.end()) throw EngineError(DZN_E_MISSING, "missing state_dict key: " + key);
  h->used.insert(key);
  return it->second;
}

void expect_numel(const HostT& t, int64_t n, const std::string& key) {
  if ((int64_t)t.v.size() != n)
    throw EngineError(DZN_E_INVALID, "shape mismatch for " + key + ": got " +
                                         std::to_string(t.v.size()) + " elements, expected " +
                                         std::to_string(n));
}

// W given as [N][K] row-major (already in the contraction's k order); pads to [Np][Kp]
Lin make_lin(H* h, const std::vector<float>& W, const float* bias, int N, int K, int Np, int Kp) {
  std::vector<float> wp((size_t)Np * Kp, 0.f);
  for (int n = 0; n < N; ++n)
    std::copy(W.begin() + (size_t)n * K, W.begin() + (size_t)(n + 1) * K, wp.begin() + (size_t)n * Kp);
  Lin l;
  l.N = Np;
  l.K = Kp;
  l.Nt = N;
  l.Kt = K;
  l.W = upload(h, wp);
  if (prec_is_split(h->cfg.precision) && Kp % 32 == 0) {
    l.W3 = dalloc<u16>(h, (int64_t)3 * Np * Kp, false);
    if (launch_split_weights(l.W, Np, Kp, Kp, l.W3, nullptr) != DZN_OK)
      throw EngineError(DZN_E_HIP, "split_weights launch failed");
    if (prec_is_h2(h->cfg.precision)) {
      l.W2h = dalloc<u16>(h, (int64_t)2 * Np * Kp, false);
      l.wsc = dalloc<float>(h, Np, false);
      if (launch_split_weights_h2(l.W, Np, Kp, Kp, l.W2h, l.wsc, nullptr) != DZN_OK)
        throw EngineError(DZN_E_HIP, "split_weights_h2 launch failed");
    }
    if (h->cfg.precision == DZN_PREC_F16 && h->mx_pack && h->sw.f16_mx) {
      l.Wmx = dalloc<unsigned char>(h, (int64_t)4 * Np * Kp, false);
      l.wsc_mx = dalloc<float>(h, Np, false);
      if (launch_split_weights_mx(l.W, Np, Kp, Kp, l.Wmx, l.wsc_mx, nullptr) != DZN_OK)
        throw EngineError(DZN_E_HIP, "split_weights_mx launch failed");
    }
    HIPCHK(hipDeviceSynchronize());
  }
  if (bias) {
    std::vector<float> bp(Np, 0.f);
    std::copy(bias, bias + N, bp.begin());
    l.b = upload(h, bp);
  }
  return l;
}

Lin linear_from_sd(H* h, const std::string& prefix, int N, int K, int Np, int Kp, bool bias = true) {
  const HostT& w = need(h, prefix + ".weight");
  expect_numel(w, (int64_t)N * K, prefix + ".weight");
  const float* b = nullptr;
  if (bias) {
    const HostT& bt = need(h, prefix + ".bias");
    expect_numel(bt, N, prefix + ".bias");
    b = bt.v.data();
  }
  return make_lin(h, w.v, b, N, K, Np, Kp);
}

// y = LN(x; gamma, beta) W^T + bias  ==  rstd (x W'^T - mean colsum(W')) + (bias + W beta),  W' = W diag(gamma):
// the contraction reads the RAW rows and its epilogue finishes the norm from (mean, rstd) per row
// (dzn_gemm_desc.ln_stats).  Used where a LayerNorm feeds only linears (pre-norm encoder layers
// W2V/components.py:920-935, feature projection :305-306, Conformer sub-blocks conformer.py:136-214).
Lin make_lin_ln(H* h, const std::vector<float>& W, const float* bias, const std::vector<float>& gamma,
                const std::vector<float>& beta, int N, int K, int Np, int Kp) {
  std::vector<float> wf((size_t)N * K), bf(N), cs(Np, 0.f);
  for (int n = 0; n < N; ++n) {
    double sb = bias ? (double)bias[n] : 0.0, sc = 0.0;
    for (int k = 0; k < K; ++k) {
      const float w = W[(size_t)n * K + k];
      const float wg = w * gamma[k];
      wf[(size_t)n * K + k] = wg;
      sc += (double)wg;
      sb += (double)w * (double)beta[k];
    }
    bf[n] = (float)sb;
    cs[n] = (float)sc;
  }
  Lin l = make_lin(h, wf, bf.data(), N, K, Np, Kp);
  l.csum = upload(h, cs);
  return l;
}

LNp ln_from_sd(H* h, const std::string& prefix, int Cn) {
  const HostT& g = need(h, prefix + ".weight");
  const HostT& b = need(h, prefix + ".bias");
  expect_numel(g, Cn, prefix + ".weight");
  expect_numel(b, Cn, prefix + ".bias");
  LNp l;
  l.C = Cn;
  l.g = upload(h, g.v);
  l.b = upload(h, b.v);
  return l;
}

// The one loader of a NormLin: W [N][K] / bias as host vectors, the norm over K at ln_prefix ("" = no norm in front), and the
// fold decision.  `loaded`: the norm's device copy where the caller has uploaded it already.
NormLin norm_lin(H* h, const std::vector<float>& W, const float* bias, const std::string& ln_prefix, bool fold, int N, int K,
                 int Np, int Kp, const LNp* loaded = nullptr) {
  NormLin nl;
  if (!ln_prefix.empty()) nl.ln = loaded ? *loaded : ln_from_sd(h, ln_prefix, K);
  nl.folded = fold && nl.ln.C > 0;
  nl.lin = nl.folded ? make_lin_ln(h, W, bias, need(h, ln_prefix + ".weight").v, need(h, ln_prefix + ".bias").v, N, K, Np, Kp)
                     : make_lin(h, W, bias, N, K, Np, Kp);
  return nl;
}

NormLin norm_lin_from_sd(H* h, const std::string& prefix, const std::string& ln_prefix, bool fold, int N, int K, int Np, int Kp,
                         const LNp* loaded = nullptr) {
  LNp ln;
  if (!ln_prefix.empty()) ln = loaded ? *loaded : ln_from_sd(h, ln_prefix, K);
  const HostT& w = need(h, prefix + ".weight");
  const HostT& bt = need(h, prefix + ".bias");
  expect_numel(w, (int64_t)N * K, prefix + ".weight");
  expect_numel(bt, N, prefix + ".bias");
  return norm_lin(h, w.v, bt.v.data(), ln_prefix, fold, N, K, Np, Kp, &ln);
}

// q/k/v as one contraction: the three [rows, K] weights stacked to [3 rows, K], the biases to [3 rows]
std::pair<std::vector<float>, std::vector<float>> stack_qkv(H* h, const std::string& q, const std::string& k, const std::string& v,
                                                            int rows, int K) {
  std::vector<float> W((size_t)3 * rows * K), bias((size_t)3 * rows);
  const std::string* names[3] = {&q, &k, &v};
  for (int t = 0; t < 3; ++t) {
    const HostT& w = need(h, *names[t] + ".weight");
    const HostT& b = need(h, *names[t] + ".bias");
    expect_numel(w, (int64_t)rows * K, *names[t] + ".weight");
    expect_numel(b, rows, *names[t] + ".bias");
    std::copy(w.v.begin(), w.v.end(), W.begin() + (size_t)t * rows * K);
    std::copy(b.v.begin(), b.v.end(), bias.begin() + (size_t)t * rows);
  }
  return {std::move(W), std::move(bias)};
}

int conv_out(int n, int k, int s) { return n < k ? 0 : (n - k) / s + 1; }

// W2V/components.py:641-666
int relpos_bucket(int rel, int num_buckets, int max_distance) {
  const int nb = num_buckets / 2;
  int ret = rel > 0 ? nb : 0;
  const int a = rel < 0 ? -rel : rel;
  const int max_exact = nb / 2;
  if (a < max_exact) return ret + a;
  const float v = logf((float)a / (float)max_exact) /
                  (float)std::log((double)max_distance / (double)max_exact) *
                  (float)(nb - max_exact);
  long large = max_exact + (long)v;
  if (large > nb - 1) large = nb - 1;
  return ret + (int)large;
}

// ------------------------------------------------------------------ segmentation: finalize
void finalize_seg(H* h) {
  const dzn_config& c = h->cfg;
  const std::string P = "wavlm_model.";
  const bool fold = h->sw.fold_ln;
  h->nconv = c.n_conv;
  h->D = c.embed_dim;
  h->H = c.total_heads;
  h->A = c.attention_in;
  h->Fh = c.ffn_hidden;
  if (c.n_conv < 1 || c.n_conv > DZN_MAX_CONV || c.n_layers < 1 || c.n_layers > DZN_MAX_LAYERS ||
      c.total_heads > DZN_MAX_HEADS || c.embed_dim != c.total_heads * 64 || (c.attention_in % 32) ||
      (c.ffn_hidden % 32) || c.attention_in != c.conf_heads * 64 ||
      c.embed_dim % c.pos_conv_groups || ((c.embed_dim / c.pos_conv_groups) % 8))
    throw EngineError(DZN_E_INVALID, "unsupported architecture (head_dim must be 64, dims % 32)");
  if (c.max_speakers_per_chunk > 8 || c.n_classes > 16)
    throw EngineError(DZN_E_INVALID, "powerset too large");
  for (int i = 0; i < c.n_conv; ++i) {
    h->C[i] = c.conv_ch[i];
    h->Cp[i] = pad32(c.conv_ch[i]);
  }
  // conv0
  {
    const std::string pre = P + "feature_extractor.conv_layers.0";
    const HostT& w = need(h, pre + ".conv.weight");
    expect_numel(w, (int64_t)h->C[0] * c.conv_k[0], pre + ".conv.weight");
    h->conv0_w = upload(h, w.v);
    h->conv_ln[0] = ln_from_sd(h, pre + ".layer_norm", h->C[0]);
    if (c.extractor_layer_norm && c.conv_k[0] <= 10 && h->sw.conv0_quad_stats) {
      // LayerNorm statistics of conv0's frames as a quadratic form of the input samples (frontend.hip)
      std::vector<float> lq(110);
      conv0_lnq_factor(w.v.data(), h->C[0], c.conv_k[0], lq.data());
      h->conv0_lnq = upload(h, lq);
    }
    if (c.extractor_layer_norm) {   // |LN(x)_c| <= sqrt(C - 1), |GELU(t)| <= |t|
      float mg = 0.f, mb = 0.f;
      for (float v : need(h, pre + ".layer_norm.weight").v) mg = std::max(mg, std::fabs(v));
      for (float v : need(h, pre + ".layer_norm.bias").v) mb = std::max(mb, std::fabs(v));
      h->conv0_bound = std::sqrt((float)h->C[0]) * mg + mb;
    }
  }
  for (int i = 1; i < c.n_conv; ++i) {
    const std::string pre = P + "feature_extractor.conv_layers." + std::to_string(i);
    const HostT& w = need(h, pre + ".conv.weight");
    const int ci = h->C[i - 1], co = h->C[i], k = c.conv_k[i], cip = h->Cp[i - 1];
    expect_numel(w, (int64_t)co * ci * k, pre + ".conv.weight");
    std::vector<float> wp((size_t)co * k * cip, 0.f);  // [co][j*cip + ci] = w[co][ci][j]
    for (int o = 0; o < co; ++o)
      for (int ii = 0; ii < ci; ++ii)
        for (int j = 0; j < k; ++j)
          wp[((size_t)o * k + j) * cip + ii] = w.v[((size_t)o * ci + ii) * k + j];
    h->conv[i] = make_lin(h, wp, nullptr, co, k * cip, h->Cp[i], k * cip);
    h->conv[i].Kt = k * ci;
    if (c.extractor_layer_norm) h->conv_ln[i] = ln_from_sd(h, pre + ".layer_norm", co);
    if (i == 1 && prec_is_h2(c.precision) && c.extractor_layer_norm && h->conv0_lnq && c.conv_k[0] == 10 &&
        c.conv_s[0] == 5 && k == 3 && c.conv_s[1] == 2 && h->C[0] % 64 == 0 && h->C[0] >= 128 &&
        h->Cp[0] == h->C[0] && h->Cp[1] == 160 && h->sw.fuse_conv01) {
      // (C[0] >= 128: with a single 64-channel slab the kernel's epilogue statistics would race, frontend_fused.hip)
      h->conv1_W2f = dalloc<u16>(h, (int64_t)2 * h->Cp[1] * k * cip, false);
      h->conv1_wscf = dalloc<float>(h, h->Cp[1], false);
      if (launch_split_weights_h2_frag(h->conv[1].W, h->Cp[1], k * cip, h->conv1_W2f, h->conv1_wscf, nullptr) != DZN_OK)
        throw EngineError(DZN_E_HIP, "split_weights_h2_frag launch failed");
      HIPCHK(hipDeviceSynchronize());
    }
  }
  const int last = c.n_conv - 1;
  {
    const HostT& dw = need(h, P + "feature_extractor.dummy_weight");
    expect_numel(dw, h->C[last], "dummy_weight");
    h->dummy_w = upload(h, dw.v);
  }
  const int D = h->D;
  h->fp = norm_lin_from_sd(h, P + "encoder.feature_projection.projection", P + "encoder.feature_projection.layer_norm", fold,
                           D, h->C[last], D, h->Cp[last]);
  // positional conv: fold weight norm  W = g * v / ||v||_{dims 0,1}   (components.py:344)
  {
    const std::string pc = P + "encoder.transformer.pos_conv_embed.conv";
    const HostT& g = need(h, pc + ".parametrizations.weight.original0");
    const HostT& v = need(h, pc + ".parametrizations.weight.original1");
    const HostT& b = need(h, pc + ".bias");
    const int K = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G;
    expect_numel(g, K, pc + ".original0");
    expect_numel(v, (int64_t)D * cg * K, pc + ".original1");
    expect_numel(b, D, pc + ".bias");
    std::vector<double> nrm(K, 0.0);
    for (int o = 0; o < D; ++o)
      for (int ii = 0; ii < cg; ++ii)
        for (int j = 0; j < K; ++j) {
          const double t = v.v[((size_t)o * cg + ii) * K + j];
          nrm[j] += t * t;
        }
    // split modes: groups whose width is not a multiple of 32 (base: 768 / 16 = 48) are zero-padded to the next one
    // (64) in the weights AND in the pre-split padded copy of x, so the contraction keeps whole 32-k tiles per tap and
    // runs on the fp16 / bf16 planes instead of the fp32 MFMA fallback (r2: 15 % of BASELINE configs[1])
    const int cgp = prec_is_split(c.precision) ? round_up(cg, 32) : cg;
    h->pos_cgp = cgp;
    h->posconv_resident = h->sw.posconv_resident && c.precision == DZN_PREC_F32_H2 && cgp == 64;
    std::vector<float> wp((size_t)D * K * cgp, 0.f);
    for (int o = 0; o < D; ++o)
      for (int ii = 0; ii < cg; ++ii)
        for (int j = 0; j < K; ++j) {
          const float nj = (float)std::sqrt(nrm[j]);
          wp[((size_t)o * K + j) * cgp + ii] = g.v[j] * v.v[((size_t)o * cg + ii) * K + j] / nj;
        }
    h->posconv = make_lin(h, wp, b.v.data(), D, K * cgp, D, K * cgp);
    h->posconv.Kt = K * cg;
  }
  if (!c.layer_norm_first) h->enc_ln = ln_from_sd(h, P + "encoder.transformer.layer_norm", D);
  h->layers.resize(c.n_layers);
  int maxQ = 64, maxF = 32;
  for (int i = 0; i < c.n_layers; ++i) {
    EncLayer& L = h->layers[i];
    const std::string lp = P + "encoder.transformer.layers." + std::to_string(i);
    L.attn = c.use_attention[i] && c.n_heads[i] > 0;
    L.ffn = c.use_ffn[i] != 0;
    L.pre_norm = c.layer_norm_first != 0;
    L.ln1 = ln_from_sd(h, lp + ".layer_norm", D);
    L.ln2 = ln_from_sd(h, lp + ".final_layer_norm", D);
    if (L.attn) {
      L.h = c.n_heads[i];
      const int hd = L.h * 64;
      maxQ = std::max(maxQ, hd);
      const auto wb = stack_qkv(h, lp + ".attention.q_proj", lp + ".attention.k_proj", lp + ".attention.v_proj", hd, D);
      L.qkv = norm_lin(h, wb.first, wb.second.data(), L.pre_norm ? lp + ".layer_norm" : "", fold, 3 * hd, D, 3 * hd, D, &L.ln1);
      L.out = linear_from_sd(h, lp + ".attention.out_proj", D, hd, D, hd);
      const HostT& wg = need(h, lp + ".attention.gru_rel_pos_linear.weight");
      const HostT& bg = need(h, lp + ".attention.gru_rel_pos_linear.bias");
      const HostT& cs = need(h, lp + ".attention.gru_rel_pos_const");
      expect_numel(wg, 8 * 64, "gru_rel_pos_linear.weight");
      expect_numel(bg, 8, "gru_rel_pos_linear.bias");
      expect_numel(cs, h->H, "gru_rel_pos_const");
      L.Wg = upload(h, wg.v);
      L.bg = upload(h, bg.v);
      L.cst = upload(h, cs.v);
      std::vector<int32_t> hi(c.head_idx[i], c.head_idx[i] + L.h);
      for (int v : hi)
        if (v < 0 || v >= h->H) throw EngineError(DZN_E_INVALID, "head index out of range");
      L.head_idx = dalloc<int32_t>(h, L.h, false);
      HIPCHK(hipMemcpy(L.head_idx, hi.data(), L.h * sizeof(int32_t), hipMemcpyHostToDevice));
      if (i == 0) {
        const HostT& e = need(h, lp + ".attention.rel_attn_embed.weight");
        expect_numel(e, (int64_t)c.num_buckets * h->H, "rel_attn_embed.weight");
        h->rel_embed = e.v;
      }
    }
    if (L.ffn) {
      L.F = c.ffn_dim[i];
      L.Fp = pad32(L.F);
      maxF = std::max(maxF, L.Fp);
      L.f1 = norm_lin_from_sd(h, lp + ".feed_forward.intermediate_dense", L.pre_norm ? lp + ".final_layer_norm" : "", fold, L.F, D,
                              L.Fp, D, &L.ln2);
      L.f2 = linear_from_sd(h, lp + ".feed_forward.output_dense", D, L.F, D, L.Fp);
    }
  }
  if (h->rel_embed.empty())
    throw EngineError(DZN_E_INVALID, "layer 0 must carry attention (rel_attn_embed lives there)");
  {
    // LayerNorm statistics from the epilogue of the contraction that writes the rows (dzn_gemm_desc.stat_partial): LN2's from
    // out_proj, and LN1's of layer i from the FFN-down of layer i - 1.  Layer 0 (rows from the positional conv), a layer behind
    // one without an FFN, post-norm models and unfolded norms keep the pass over the rows (gate_stats / row_stats).
    bool any = false;
    for (int i = 0; i < c.n_layers; ++i) {
      EncLayer& L = h->layers[i];
      if (!h->sw.epilogue_stats) break;
      any = any || (L.attn && L.ffn && L.f1.folded);
      if (i == 0 || !L.pre_norm || !h->layers[i - 1].ffn) continue;
      L.stats_in = L.attn ? (L.qkv.folded && D == h->H * 64 && h->H <= 16) : (L.ffn && L.f1.folded);
      any = any || L.stats_in;
    }
    // spart holds 32 partials per row; a contraction over N = D columns leaves one per wavefront tile, the narrowest of which
    // (any family, any forced tile) is 32 columns wide in 64-column steps
    if (any && 2 * ((D + 63) / 64) > 32)
      throw EngineError(DZN_E_INVALID, "encoder_embed_dim > 1024: the epilogue's row statistics need more than 32 partials per row "
                                       "(DZN_NO_EPILOGUE_STATS=1 runs without them)");
  }
  {
    const HostT& w = need(h, "weight_sum.weight");
    expect_numel(w, c.n_layers + 1, "weight_sum.weight");
    h->wsum_w = w.v;
  }
  const int A = h->A, Fh = h->Fh;
  h->proj = linear_from_sd(h, "proj", A, D, A, D);
  h->lnorm = ln_from_sd(h, "lnorm", A);
  h->conf.resize(c.conf_layers);
  for (int i = 0; i < c.conf_layers; ++i) {
    ConfLayer& L = h->conf[i];
    const std::string cp = "conformer.conformer_layer." + std::to_string(i);
    L.ffn1_w1 = norm_lin_from_sd(h, cp + ".ffn1.w_1", cp + ".ffn1.ln_norm", fold, Fh, A, Fh, A);
    L.ffn1_w2 = linear_from_sd(h, cp + ".ffn1.w_2", A, Fh, A, Fh);
    L.ffn2_w1 = norm_lin_from_sd(h, cp + ".ffn2.w_1", cp + ".ffn2.ln_norm", fold, Fh, A, Fh, A);
    L.ffn2_w2 = linear_from_sd(h, cp + ".ffn2.w_2", A, Fh, A, Fh);
    {
      const LNp ln = ln_from_sd(h, cp + ".mha.ln_norm", A);
      const auto wb = stack_qkv(h, cp + ".mha.mha.linearQ", cp + ".mha.mha.linearK", cp + ".mha.mha.linearV", A, A);
      L.qkv = norm_lin(h, wb.first, wb.second.data(), cp + ".mha.ln_norm", fold, 3 * A, A, 3 * A, A, &ln);
    }
    L.o = linear_from_sd(h, cp + ".mha.mha.linearO", A, A, A, A);
    L.pw1 = norm_lin_from_sd(h, cp + ".conv.pointwise_conv1", cp + ".conv.ln_norm", fold, 2 * A, A, 2 * A, A);
    L.pw2 = linear_from_sd(h, cp + ".conv.pointwise_conv2", A, A, A, A);
    {
      // fold eval BatchNorm1d into the depthwise taps (conformer.py:205)
      const int ks = c.conf_kernel;
      const HostT& w = need(h, cp + ".conv.depthwise_conv.weight");
      const HostT& b = need(h, cp + ".conv.depthwise_conv.bias");
      const HostT& g = need(h, cp + ".conv.bn_norm.weight");
      const HostT& be = need(h, cp + ".conv.bn_norm.bias");
      const HostT& rm = need(h, cp + ".conv.bn_norm.running_mean");
      const HostT& rv = need(h, cp + ".conv.bn_norm.running_var");
      expect_numel(w, (int64_t)A * ks, cp + ".conv.depthwise_conv.weight");
      std::vector<float> wf((size_t)A * ks), bf(A);
      for (int ch = 0; ch < A; ++ch) {
        const float s = g.v[ch] / std::sqrt(rv.v[ch] + 1e-5f);
        for (int j = 0; j < ks; ++j) wf[(size_t)ch * ks + j] = w.v[(size_t)ch * ks + j] * s;
        bf[ch] = (b.v[ch] - rm.v[ch]) * s + be.v[ch];
      }
      L.dw = upload(h, wf);
      L.dwb = upload(h, bf);
    }
    L.out_ln = ln_from_sd(h, cp + ".ln_norm", A);
  }
  {
    const HostT& w = need(h, "classifier.weight");
    const HostT& b = need(h, "classifier.bias");
    expect_numel(w, (int64_t)c.n_classes * A, "classifier.weight");
    expect_numel(b, c.n_classes, "classifier.bias");
    h->cls_w = upload(h, w.v);
    h->cls_b = upload(h, b.v);
    // PA/utils/powerset.py:68-97: classes ordered by set size, then lexicographic combinations
    const int S = c.max_speakers_per_chunk;
    std::vector<uint8_t> map;
    int rows = 0;
    for (int size = 0; size <= c.max_speakers_per_frame; ++size) {
      std::vector<int> idx(size);
      for (int i = 0; i < size; ++i) idx[i] = i;
      while (true) {
        std::vector<uint8_t> r(S, 0);
        for (int v : idx) r[v] = 1;
        map.insert(map.end(), r.begin(), r.end());
        ++rows;
        int i = size - 1;
        while (i >= 0 && idx[i] == S - size + i) --i;
        if (i < 0) break;
        ++idx[i];
        for (int j = i + 1; j < size; ++j) idx[j] = idx[j - 1] + 1;
      }
    }
    if (rows != c.n_classes) throw EngineError(DZN_E_INVALID, "n_classes != powerset size");
    h->mapping = dalloc<uint8_t>(h, (int64_t)map.size(), false);
    HIPCHK(hipMemcpy(h->mapping, map.data(), map.size(), hipMemcpyHostToDevice));
  }

  // ---- workspace for (max_batch, max_samples) ----
  const int64_t B = c.max_batch;
  int n = c.max_samples;
  int64_t maxbuf = 0;
  for (int i = 0; i < c.n_conv; ++i) {
    n = conv_out(n, c.conv_k[i], c.conv_s[i]);
    h->maxT[i] = n;
    maxbuf = std::max(maxbuf, (int64_t)B * n * h->Cp[i]);
  }
  h->maxL = n;
  if (n < 1) throw EngineError(DZN_E_INVALID, "max_samples too short");
  const int64_t ML = B * n;
  h->stats = dalloc<float>(h, B * 2);
  if (!c.extractor_layer_norm) h->gn_stats = dalloc<float>(h, gn_stats_floats((int)B, h->maxT[0], h->C[0], h->Cp[0]));
  h->bufA = dalloc<float>(h, maxbuf);
  {
    // bufB holds every odd conv output (and the feature-projection LN output)
    int64_t need_b = B * n * h->Cp[c.n_conv - 1];
    for (int i = 1; i < c.n_conv; i += 2) need_b = std::max(need_b, B * h->maxT[i] * h->Cp[i]);
    h->bufB = dalloc<float>(h, need_b);
  }
  h->x = dalloc<float>(h, ML * D);
  h->xpad = dalloc<float>(h, B * (n + c.pos_conv_kernel) * D);
  if (prec_is_split(c.precision)) {
    h->xpad3_plane = B * (n + c.pos_conv_kernel) * (int64_t)(c.pos_conv_groups * round_up(D / c.pos_conv_groups, 32));
    h->xpad3 = dalloc<u16>(h, 3 * h->xpad3_plane);
  }
  h->y = dalloc<float>(h, ML * D);
  h->ws = dalloc<float>(h, ML * D);
  // the per-layer buffers of the deferred layer-weighted sum are OPTIONAL: they are taken last, by alloc_optional_workspace()
  h->xl_elems = (c.layer_norm_first && fold && c.n_layers > 0 && c.n_layers < WS_SUM_MAX && D % 4 == 0 &&
                 h->sw.ws_defer) ? (int64_t)c.n_layers * ML * D : 0;
  h->qkv = dalloc<float>(h, ML * 3 * maxQ);
  if (c.precision == DZN_PREC_F32_H2 && maxQ > 0 && h->sw.att_planes) {
    // two fp16 planes of [rows + 64][2 * maxQ] (the bytes of the fp32 K / V they replace) and the slot scales; zero-filled once:
    // the 64 rows past a batch are only ever read for keys that are masked, but they must be finite
    h->kvp_rows = ML + 64;
    h->kvp_ldmax = 2 * maxQ;
    h->kvp = dalloc<uint16_t>(h, 2 * h->kvp_rows * h->kvp_ldmax);
    h->kvs = dalloc<float>(h, h->kvp_rows * (h->kvp_ldmax / 64));
  }
  h->ao = dalloc<float>(h, ML * maxQ);
  h->gate = dalloc<float>(h, ML * h->H);
  h->mid = dalloc<float>(h, ML * maxF);
  h->hz = dalloc<float>(h, ML * A);
  h->ht = dalloc<float>(h, ML * A);
  h->hmid = dalloc<float>(h, ML * std::max(Fh, 3 * A));
  h->hv = dalloc<float>(h, ML * A);
  h->rstat = dalloc<float>(h, ML * 2);
  h->spart = dalloc<float>(h, ML * 32 * 2);
  h->amax = dalloc<float>(h, (int64_t)dzn_handle::AM_COUNT * c.max_batch);
}

// Optional workspace, taken AFTER everything a forward needs (segmentation + embedding) and only against a reserve, so that
// several handles on one device (DiariZenPipeline num_streams, bench config1) cannot starve what is allocated later — torch's
// waveform / chunk copies, VBx, RCCL (the r4 gate was `need < free / 2` per handle at a point where the embedding
// workspace did not exist yet).  A failed hipMalloc leaves the read-modify-write path in place instead of failing the handle.
void alloc_optional_workspace(H* h) {
  if (h->xl_elems <= 0) return;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
  const int64_t need = h->xl_elems * (int64_t)sizeof(float);
  const int64_t reserve = std::max<int64_t>((int64_t)32 << 30, (int64_t)(total_b / 4));   // stays free after the allocation
  if (need + reserve > (int64_t)free_b) return;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)need) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  h->allocs.push_back(p);
  h->bytes += need;
  h->xl = reinterpret_cast<float*>(p);
}

// ------------------------------------------------------------------ embedding: finalize
// kaldi fbank at 16 kHz: 25 ms frames every 10 ms, a frame row zero-padded to a multiple of 32 columns, a 512-point real DFT
// of which bins 0 .. 255 are kept (the spectrum row is [cos | sin] of those bins)
constexpr int FB_FLEN = 400, FB_SHIFT = 160, FB_KP = 416, FB_NFFT = 512, FB_BINS = 256;

// The four trunk stages g[0 .. 4) over an fbank image of NB mel bins x T frames: stage 0 keeps its size, every later stage
// halves both sides (3x3, stride 2, padding 1).  The tables are left null.
void stage_geometry(int NB, int T, const int* C, EmbStage* g) {
  for (int s = 0; s < 4; ++s) {
    const int Hs = s == 0 ? NB : (g[s - 1].Hs - 1) / 2 + 1, Ws = s == 0 ? T : (g[s - 1].Ws - 1) / 2 + 1;
    g[s] = {s, Hs, Ws, C[s], (int64_t)(Hs + 2) * (Ws + 2) * C[s], ((int64_t)(Ws + 2) + 1) * C[s], Hs * Ws, nullptr, nullptr};
  }
}

void fold_bn(H* h, const std::string& bn, int Cn, std::vector<float>& scale, std::vector<float>& shift) {
  const HostT& g = need(h, bn + ".weight");
  const HostT& b = need(h, bn + ".bias");
  const HostT& rm = need(h, bn + ".running_mean");
  const HostT& rv = need(h, bn + ".running_var");
  expect_numel(g, Cn, bn + ".weight");
  scale.resize(Cn);
  shift.resize(Cn);
  for (int i = 0; i < Cn; ++i) {
    scale[i] = g.v[i] / std::sqrt(rv.v[i] + 1e-5f);
    shift[i] = b.v[i] - rm.v[i] * scale[i];
  }
}

// One conv of the ResNet with its BatchNorm folded: the weights OIHW [cout][cin][ksz][ksz] times the BatchNorm scale of their
// output channel as K = ksz^2 cin columns of the contraction's rows, wp[o * ld + (dh * ksz + dw) * cin + ci]; returns the shifts.
std::vector<float> conv_bn_columns(H* h, const std::string& conv, const std::string& bn, int cin, int cout, int ksz, float* wp,
                                   int ld) {
  const HostT& w = need(h, conv + ".weight");
  expect_numel(w, (int64_t)cout * cin * ksz * ksz, conv + ".weight");
  std::vector<float> sc, sh;
  fold_bn(h, bn, cout, sc, sh);
  for (int o = 0; o < cout; ++o)
    for (int ci = 0; ci < cin; ++ci)
      for (int dh = 0; dh < ksz; ++dh)
        for (int dw = 0; dw < ksz; ++dw)
          wp[(size_t)o * ld + (dh * ksz + dw) * cin + ci] = w.v[(((size_t)o * cin + ci) * ksz + dh) * ksz + dw] * sc[o];
  return sh;
}

ResConv make_resconv(H* h, const std::string& conv, const std::string& bn, int cin, int cout, int ksz,
                     int stride) {
  const int K = ksz * ksz * cin;
  std::vector<float> wp((size_t)cout * K);
  const std::vector<float> sh = conv_bn_columns(h, conv, bn, cin, cout, ksz, wp.data(), K);
  ResConv r;
  r.cin = cin;
  r.cout = cout;
  r.ksz = ksz;
  r.stride = stride;
  r.l = make_lin(h, wp, sh.data(), cout, K, cout, K);
  for (int o = 0; o < cout; ++o) {
    double l1 = 0.0;
    for (int k = 0; k < K; ++k) l1 += std::fabs((double)wp[(size_t)o * K + k]);
    r.l1max = std::max(r.l1max, (float)(l1 * (1.0 + 1e-6)));
    r.bmax = std::max(r.bmax, std::fabs(sh[o]));
  }
  return r;
}

// conv2 (3x3, stride 1, cout -> cout) of a down-sampling block with the block's 1x1 stride-2 shortcut (cprev -> cout) folded
// in: out = relu(conv2(mid) + b2 + Ws x_centre + bs) is ONE sum over K = 9 cout + cprev.  Weight row = [W2 | Ws | 0-pad to a
// multiple of 64], bias = b2 + bs, both with their BatchNorm folded; the planes and their per-row scales are taken over the
// whole concatenated row (make_lin).  Built once: the weights do not change between calls.
ResConv make_resconv_shortcut(H* h, const std::string& conv, const std::string& bn, const std::string& sconv,
                              const std::string& sbn, int cprev, int cout) {
  const int K1 = 9 * cout, Kp = K1 + (cprev + 63) / 64 * 64;
  std::vector<float> wp((size_t)cout * Kp, 0.f);
  std::vector<float> bias = conv_bn_columns(h, conv, bn, cout, cout, 3, wp.data(), Kp);
  const std::vector<float> ssh = conv_bn_columns(h, sconv, sbn, cprev, cout, 1, wp.data() + K1, Kp);
  if (K1 % 64 != 0 || cprev % 32 != 0) throw EngineError(DZN_E_INVALID, "shortcut fusion: channel counts");
  for (int o = 0; o < cout; ++o) bias[o] += ssh[o];
  ResConv r;
  r.cin = cout;
  r.cout = cout;
  r.k2 = cprev;
  r.l = make_lin(h, wp, bias.data(), cout, Kp, cout, Kp);
  r.l.Kt = K1 + cprev;   // algorithmic flops: the columns that exist
  return r;
}

void finalize_emb(H* h) {
  const dzn_config& c = h->cfg;
  const std::string E = "embedding.resnet.";
  const int NB = c.num_mel_bins;
  if (NB != 80 || c.embed_out_dim <= 0) throw EngineError(DZN_E_INVALID, "embedding config");
  {
    // torch.hamming_window(400, periodic=False): 0.54 - 0.46 cos(2 pi n / (N-1))
    std::vector<float> wdw(FB_FLEN);
    for (int i = 0; i < FB_FLEN; ++i)
      wdw[i] = (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * (double)i / (double)(FB_FLEN - 1)));
    h->hamming = upload(h, wdw);
    // real DFT as a contraction: rows 0..255 cos, 256..511 sin, bins 0..255 (bin 256 unused)
    std::vector<float> dft((size_t)2 * FB_BINS * FB_KP, 0.f);
    for (int f = 0; f < FB_BINS; ++f)
      for (int t = 0; t < FB_FLEN; ++t) {
        const double ang = 2.0 * M_PI * (double)((int64_t)f * t % FB_NFFT) / (double)FB_NFFT;
        dft[(size_t)f * FB_KP + t] = (float)std::cos(ang);
        dft[(size_t)(FB_BINS + f) * FB_KP + t] = (float)(-std::sin(ang));
      }
    h->dft = make_lin(h, dft, nullptr, 2 * FB_BINS, FB_KP, 2 * FB_BINS, FB_KP);
    // Kaldi mel banks (torchaudio.compliance.kaldi.get_mel_banks, float32 arithmetic):
    // low 20 Hz, high = Nyquist, 80 triangles in mel(f) = 1127 ln(1 + f/700), bins 0..255
    const float mel_low = 1127.0f * logf(1.0f + 20.0f / 700.0f);
    const float mel_high = 1127.0f * logf(1.0f + 8000.0f / 700.0f);
    const float delta = (mel_high - mel_low) / (float)(NB + 1);
    std::vector<float> mw((size_t)NB * FB_BINS, 0.f);
    for (int b = 0; b < NB; ++b) {
      const float left = mel_low + (float)b * delta;
      const float center = mel_low + ((float)b + 1.0f) * delta;
      const float right = mel_low + ((float)b + 2.0f) * delta;
      for (int f = 0; f < FB_BINS; ++f) {
        const float mel = 1127.0f * logf(1.0f + (31.25f * (float)f) / 700.0f);
        const float up = (mel - left) / (center - left);
        const float down = (right - mel) / (right - center);
        mw[(size_t)b * FB_BINS + f] = std::max(0.0f, std::min(up, down));
      }
    }
    h->mel = make_lin(h, mw, nullptr, NB, FB_BINS, NB, FB_BINS);
  }
  const int m = 32;
  {
    std::vector<float> wf((size_t)m * 9);
    const std::vector<float> sh = conv_bn_columns(h, E + "conv1", E + "bn1", 1, m, 3, wf.data(), 9);
    h->stem_w = upload(h, wf);
    h->stem_b = upload(h, sh);
  }
  const int nblocks[4] = {3, 4, 6, 3};
  h->stages.resize(4);
  // DZN_PREC_F16: bit CLS_RESNET of DZN_F16_KEEP2 governs the whole trunk — the contractions of img_desc keep two fp16 terms
  // and so do the fused BasicBlocks; without it both run on ONE term (the embedding trunk is three orders of magnitude inside
  // its cosine bar with one term: profiles/r4_reduced_mode_emulation.txt)
  const bool h2 = prec_is_h2(c.precision), keep2 = c.precision == DZN_PREC_F16 && ((h->sw.f16_keep2 >> CLS_RESNET) & 1);
  int cin = m;
  for (int s = 0; s < 4; ++s) {
    const int cout = m << s;
    h->sC[s] = cout;
    h->stages[s].resize(nblocks[s]);
    for (int j = 0; j < nblocks[s]; ++j) {
      const std::string bp = E + "layer" + std::to_string(s + 1) + "." + std::to_string(j);
      ResBlock& rb = h->stages[s][j];
      const int stride = (j == 0 && s > 0) ? 2 : 1;
      rb.c1 = make_resconv(h, bp + ".conv1", bp + ".bn1", cin, cout, 3, stride);
      const bool down = stride != 1 || cin != cout;   // with a 1x1 shortcut; DZN_NO_SHORTCUT_FUSION=1 keeps it its own launch
      if (down && h->sw.fuse_shortcut) {
        rb.c2 = make_resconv_shortcut(h, bp + ".conv2", bp + ".bn2", bp + ".shortcut.0", bp + ".shortcut.1", cin, cout);
      } else {
        rb.c2 = make_resconv(h, bp + ".conv2", bp + ".bn2", cout, cout, 3, 1);
        if (down) rb.sc = make_resconv(h, bp + ".shortcut.0", bp + ".shortcut.1", cin, cout, 1, stride);
      }
      // (r4) stride-1 blocks of 32 and 64 planes in the two-term fp16 modes: both convolutions in one kernel, the intermediate
      // image stays in LDS; DZN_NO_RESBLOCK_FUSION=1 keeps the per-conv kernels.  DZN_RESBLOCK_WS: which plane counts take the
      // producer / consumer form (bit 0: 32 planes, bit 1: 64 planes — the only fused form that stage has)
      const bool fusable = h->sw.fuse_resblock && h2 && rb.c1.l.W2h && rb.c2.l.W2h;
      const int ws = h->sw.resblock_ws;
      if (down) rb.form = rb.c2.k2 > 0 ? ResBlock::DOWN_FOLDED : ResBlock::DOWN;
      else if (fusable && cin == 32 && !(ws & 1)) rb.form = ResBlock::FUSED32;
      else if (fusable && ((cin == 32 && (ws & 1)) || (cin == 64 && (ws & 2)))) rb.form = ResBlock::WS;
      rb.np = c.precision == DZN_PREC_F16 && !keep2 ? 1 : 2;
      for (ResConv* rc : {&rb.c1, &rb.c2, &rb.sc}) {
        if (rc == &rb.sc && rb.form != ResBlock::DOWN) continue;   // no shortcut conv of its own
        // first ResNet stage: every input pixel split once instead of once per tap
        rc->c32 = prec_is_split(c.precision) && rc->cin == 32 && rc->cout == 32 && rc->l.W3;
        rc->keep2 = keep2;
      }
      cin = cout;
    }
  }
  const int feat = (m << 3) * (NB / 8) * 2;  // 256 * 10 * 2 = 5120
  h->seg1 = linear_from_sd(h, E + "seg_1", c.embed_out_dim, feat, c.embed_out_dim, feat);

  // workspace
  const int64_t B = c.max_batch;
  const int Tmax = c.max_samples < FB_FLEN ? 0 : 1 + (c.max_samples - FB_FLEN) / FB_SHIFT;
  if (Tmax < 8) throw EngineError(DZN_E_INVALID, "max_samples too short for the embedding model");
  h->maxTf = Tmax;
  // frames / spec / pw hold one pass of the fbank chain.  A pass is sized for the frame grid windows share when they lie
  // a tenth of a window apart (segmentation_step = 0.1 in every pipeline configuration): G = (B - 1) q + Tmax rows with
  // q = ceil(Tmax / 10), not B * Tmax.  Anything longer (unrelated windows, wider strides) takes several passes.
  h->fb_rows = (B - 1) * ((Tmax + 9) / 10) + Tmax;
  h->frames = dalloc<float>(h, h->fb_rows * FB_KP);
  h->spec = dalloc<float>(h, h->fb_rows * 2 * FB_BINS);
  h->pw = dalloc<float>(h, h->fb_rows * FB_BINS);
  h->fb = dalloc<float>(h, B * Tmax * NB);
  h->melg = dalloc<float>(h, B * Tmax * NB);
  EmbStage g[4];
  stage_geometry(NB, Tmax, h->sC, g);
  for (int s = 0; s < 4; ++s) {
    h->sbuf_elems[s] = g[s].img;
    for (int k = 0; k < 3; ++k) h->sbuf[s][k] = dalloc<float>(h, B * h->sbuf_elems[s]);
  }
  h->pool = dalloc<float>(h, B * 8 * feat);
  h->win_flag = dalloc<int>(h, B);
  h->win_idx = dalloc<int>(h, B);
  h->win_cnt = dalloc<int>(h, 1);
  h->emb_totals = dalloc<long long>(h, 2);
}

// bake the geometry of T fbank frames into the row-offset tables and re-zero the image borders.
// Tables are built once per T and stay on the device; a later switch back to that T is two async
// operations on the caller's stream (no host synchronisation, no upload).
void emb_set_geometry(H* h, int T, hipStream_t st) {
  if (T == h->emb_T) return;
  const int64_t B = h->cfg.max_batch;
  const bool fresh = h->geoms.find(T) == h->geoms.end();
  if (fresh && h->geoms.size() >= 64) throw EngineError(DZN_E_INVALID, "too many distinct window lengths on one handle");
  EmbStage* g = h->geoms[T].stage;
  if (fresh) stage_geometry(h->cfg.num_mel_bins, T, h->sC, g);
  for (int s = 0; s < 4; ++s) {
    if (fresh) {
      const int Hs = g[s].Hs, Ws = g[s].Ws;
      std::vector<int32_t> t1((size_t)Hs * Ws), t2((size_t)Hs * Ws, 0);
      for (int y = 0; y < Hs; ++y)
        for (int x = 0; x < Ws; ++x) {
          t1[(size_t)y * Ws + x] = (y * (Ws + 2) + x) * g[s].Cc;  // top-left of the 3x3 patch
          if (s > 0) t2[(size_t)y * Ws + x] = ((2 * y) * (g[s - 1].Ws + 2) + 2 * x) * g[s - 1].Cc;
        }
      g[s].tab1 = dalloc<int32_t>(h, (int64_t)Hs * Ws, false);
      g[s].tab2 = dalloc<int32_t>(h, (int64_t)Hs * Ws, false);
      HIPCHK(hipMemcpy(g[s].tab1, t1.data(), t1.size() * 4, hipMemcpyHostToDevice));  // synchronous, first use only
      HIPCHK(hipMemcpy(g[s].tab2, t2.data(), t2.size() * 4, hipMemcpyHostToDevice));
    }
    for (int k = 0; k < 3; ++k)
      HIPCHK(hipMemsetAsync(h->sbuf[s][k], 0, B * h->sbuf_elems[s] * sizeof(float), st));
  }
  h->stage = g;
  h->emb_T = T;
}

// ------------------------------------------------------------------ forward helpers
void chk(int rc, const char* what) {
  if (rc != DZN_OK) throw EngineError(rc, std::string("kernel launch failed: ") + what);
}

void tap(H* h, const char* name, const float* p, int64_t rows, int cols, int64_t ld, hipStream_t st) {
  if (!h->sw.debug_taps) return;
  HIPCHK(hipStreamSynchronize(st));
  std::vector<float>& v = h->taps[name];
  v.resize((size_t)rows * cols);
  HIPCHK(hipMemcpy2D(v.data(), (size_t)cols * 4, p, (size_t)ld * 4, (size_t)cols * 4, (size_t)rows,
                     hipMemcpyDeviceToHost));
}

dzn_gemm_desc gd(H* h, const float* A, const Lin& l, float* C, int64_t M, int64_t lda, int64_t ldc) {
  dzn_gemm_desc d{};
  d.A = A;
  d.W = l.W;
  d.W3 = l.W3;
  d.W2h = l.W2h;
  d.col_scale = l.wsc;
  d.Wmx = l.Wmx;
  d.col_scale_mx = l.wsc_mx;
  d.amax_count = h->cfg.max_batch;     // every tracker array has one entry per window of the largest batch (checked builds)
  d.C = C;
  d.bias = l.b;
  d.M = (int)M;
  d.N = l.N;
  d.K = l.K;
  d.lda = lda;
  d.kc = l.K;
  d.ldk = 0;
  d.ldw = l.K;
  d.ldc = ldc;
  d.alpha = 1.f;
  d.nz = 1;
  d.zdiv = 1;
  d.precision = h->cfg.precision;
  d.alg_flops = 2.0 * (double)M * l.Nt * l.Kt;  // per z
  return d;
}

void ln_t(const float* x, int64_t ldx, float* y, int64_t ldy, const LNp& p, int64_t rows,
          int Cpad, int gelu, hipStream_t st, const float* post = nullptr, float* amax = nullptr,
          int64_t amax_unit = 0) {
  chk(launch_layernorm_t(x, ldx, y, ldy, p.g, p.b, post, rows, p.C, Cpad, 1e-5f, gelu, st, amax, amax_unit),
      "layernorm");
}

// positional conv rows: m = b*L + t reads xpad[b][t .. t+Kc) — one table for all batch sizes
void ensure_pos_rowoff(H* h, int L, int Lp, int rowD, hipStream_t st) {
  if (L == h->pos_L && rowD == h->pos_rowD) return;
  h->pos_rowD = rowD;
  HIPCHK(hipStreamSynchronize(st));
  const int Bm = h->cfg.max_batch;
  std::vector<int32_t> t((size_t)Bm * L);
  for (int b = 0; b < Bm; ++b)
    for (int i = 0; i < L; ++i) t[(size_t)b * L + i] = (int32_t)(((int64_t)b * Lp + i) * h->pos_rowD);
  if (!h->pos_rowoff) h->pos_rowoff = dalloc<int32_t>(h, (int64_t)Bm * h->maxL, false);
  HIPCHK(hipMemcpy(h->pos_rowoff, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  h->pos_L = L;
}

void ensure_table(H* h, int L, hipStream_t st) {
  if (L == h->table_L) return;
  HIPCHK(hipStreamSynchronize(st));
  const int Hn = h->H, W = 2 * L - 1;
  std::vector<float> t((size_t)Hn * W);
  for (int r = -(L - 1); r <= L - 1; ++r) {
    const int bk = relpos_bucket(r, h->cfg.num_buckets, h->cfg.max_distance);
    for (int hh = 0; hh < Hn; ++hh) t[(size_t)hh * W + (r + L - 1)] = h->rel_embed[(size_t)bk * Hn + hh];
  }
  if (!h->table) h->table = dalloc<float>(h, (int64_t)Hn * (2 * h->maxL - 1), false);
  HIPCHK(hipMemcpy(h->table, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  h->table_L = L;
}

// ------------------------------------------------------------------ segmentation forward
// What the stages of one seg_forward call share.
struct SegCall {
  H* h;
  hipStream_t st;
  int B, L;
  int64_t ML;   // B * L: rows of every [B*L, .] tensor
  int stat_P = 0;   // partials per row the last FFN-down epilogue left in spart for the next layer (EncLayer::stats_in)
  // DZN_PREC_F32_H2: |max| trackers (see dzn_handle::amax).  am(slot) is NULL in the other modes, which makes
  // every contraction take its bf16 three-term / fp32 kernel.  slot < 0: a tensor without a tracker.
  float* am(int slot) const {
    return slot >= 0 && prec_is_h2(h->cfg.precision) ? h->amax + slot * (int64_t)h->cfg.max_batch : nullptr;
  }
  int conv_slot(const float* buf) const { return buf == h->bufA ? dzn_handle::AM_CONVA : dzn_handle::AM_CONVB; }
  void gemm(dzn_gemm_desc& d, F16Class cls) const {
    // DZN_PREC_F16: contraction classes that keep BOTH fp16 terms (three products) — Switches::f16_keep2 is a bit mask over
    // F16Class (default chosen from the measured sensitivity: profiles/r4_f16_sensitivity*)
    if (h->cfg.precision == DZN_PREC_F16) {
      if (!((h->sw.f16_mx >> cls) & 1)) d.Wmx = nullptr;     // single-term fp16 (or two terms, next line)
      if ((h->sw.f16_keep2 >> cls) & 1) d.precision = DZN_PREC_F32_H2;
    }
    // |max| trackers are per window: rows of a [B*L, .] tensor belong to window m / L; z-batched launches
    // (conv stack: z = window) use the z index
    // (r4 fix: a conv-stack launch with B == 1 also has nz == 1, but its rows are T_i frames of window 0, not B * L rows —
    // with unit = L its tracker index m / L ran past the one-window tracker array and scaled by whatever lay behind it)
    if ((d.nz == 1 && d.M == (int)ML) || (d.a_rowoff && d.a_rowoff == h->pos_rowoff)) d.amax_unit = L;
    chk(launch_gemm(d, st), F16_CLASSES[cls]);
  }
};

// The contraction of a NormLin over the rows `in` [ML, nl.lin.K] (tracker slot in_slot) into C, ready but for what follows
// the product: the caller adds the activation, c_amax and the residual, and launches it.
//   folded    the contraction reads `in` and finishes the norm in its epilogue from (mean, rstd) per row in rstat — left there
//             by row_stats here, unless a producer has left them already (have_stats)
//   unfolded  the stand-alone LayerNorm writes `scratch` (tracker slot scratch_slot), which the contraction reads
//   no norm   the contraction reads `in`
dzn_gemm_desc norm_lin_desc(const SegCall& s, const NormLin& nl, const float* in, int in_slot, float* scratch, int scratch_slot,
                            float* C, int64_t ldc, bool have_stats = false) {
  H* h = s.h;
  const int ld = nl.lin.K;
  if (nl.folded) {
    if (!have_stats) chk(launch_row_stats(in, ld, s.ML, nl.ln.C, 1e-5f, h->rstat, s.st), "row_stats");
  } else if (nl.ln.C > 0) {
    ln_t(in, ld, scratch, ld, nl.ln, s.ML, ld, 0, s.st, nullptr, s.am(scratch_slot), scratch_slot < 0 ? 0 : s.L);
    in = scratch;
    in_slot = scratch_slot;
  }
  dzn_gemm_desc d = gd(h, in, nl.lin, C, s.ML, ld, ldc);
  if (nl.folded) {
    d.ln_stats = h->rstat;
    d.ln_colsum = nl.lin.csum;
  }
  d.a_amax = s.am(in_slot);
  return d;
}

// Multi-head attention over packed q/k/v rows [ML, 3 * heads * 64] (tracker slot `slot`): on the fp16 K / V planes if the
// q/k/v contraction wrote them, else the split kernel in the split modes, else fp32.  Ly: the encoder layer whose gated
// relative-position bias applies; nullptr = the Conformer's plain MHSA.
void attention(const SegCall& s, const EncLayer* Ly, const float* qkv, int slot, bool planes, float* out) {
  H* h = s.h;
  const float* gate = Ly ? h->gate : nullptr;
  const float* table = Ly ? h->table : nullptr;
  const int32_t* head_idx = Ly ? Ly->head_idx : nullptr;
  const int nh = Ly ? Ly->h : h->cfg.conf_heads, Hn = Ly ? h->H : 0, hd = nh * 64;
  const char* what = Ly ? "attention" : "conf attention";
  if (planes)
    chk(launch_attention_planes(qkv, h->kvp, (s.ML + 64) * (int64_t)(2 * hd), h->kvs, 2 * hd, out, gate, table, head_idx, s.B, s.L,
                                nh, Hn, 3 * hd, hd, 0.125f, s.st, s.am(slot)),
        what);
  else if (prec_is_split(h->cfg.precision))
    chk(launch_attention_split(qkv, out, gate, table, head_idx, s.B, s.L, nh, Hn, 3 * hd, hd, 0.125f, s.st, s.am(slot)), what);
  else
    chk(launch_attention_t(qkv, out, gate, table, head_idx, s.B, s.L, nh, Hn, 3 * hd, hd, 0.125f, s.st), what);
}

// ---- conv feature extractor: T[i] frames after conv i; returns the buffer its last layer wrote ----
float* seg_conv_stack(const SegCall& s, const float* wave, int N, const int* T) {
  H* h = s.h;
  const dzn_config& c = h->cfg;
  hipStream_t st = s.st;
  const int B = s.B;
  const bool lnx = c.extractor_layer_norm != 0;
  const float* stats = nullptr;
  if (c.normalize_waveform) {
    chk(launch_wave_stats(wave, B, N, 1e-5f, h->stats, st), "wave_stats");
    stats = h->stats;
  }
  // DZN_PREC_F32_H2: conv0 + LN + GELU + conv1 in one kernel (frontend_fused.hip): conv0's 52 MB / window never
  // reach HBM.  (debug taps need the intermediate -> unfused)
  const bool fuse01 = prec_is_h2(c.precision) && lnx && h->conv1_W2f && !h->sw.debug_taps && c.n_conv > 1 && T[1] > 0;
  if (lnx && fuse01) {
  } else if (lnx) {
    chk(launch_conv0(wave, B, N, stats, h->conv0_w, h->conv_ln[0].g, h->conv_ln[0].b, h->C[0], h->Cp[0],
                     c.conv_k[0], c.conv_s[0], T[0], 1, 1e-5f, h->bufA, st, h->conv0_lnq),
        "conv0");
  } else {
    chk(launch_conv0(wave, B, N, stats, h->conv0_w, nullptr, nullptr, h->C[0], h->Cp[0], c.conv_k[0],
                     c.conv_s[0], T[0], 0, 1e-5f, h->bufA, st),
        "conv0");
    chk(launch_groupnorm_gelu(h->bufA, h->bufA, B, T[0], h->C[0], h->Cp[0], h->Cp[0], h->conv_ln[0].g,
                              h->conv_ln[0].b, 1e-5f, h->gn_stats, st, s.am(s.conv_slot(h->bufA))),
        "groupnorm");
  }
  tap(h, "conv0", h->bufA, (int64_t)B * T[0], h->C[0], h->Cp[0], st);
  float* cur = h->bufA;
  float* nxt = h->bufB;
  const int last = c.n_conv - 1;
  for (int i = 1; i < c.n_conv; ++i) {
    // conv1d(k, s) over channels-last rows: row t of the contraction starts at (t*s)*Cp_in
    dzn_gemm_desc d = gd(h, cur, h->conv[i], nxt, T[i], (int64_t)c.conv_s[i] * h->Cp[i - 1], h->Cp[i]);
    d.nz = B;
    d.a_z0 = (int64_t)T[i - 1] * h->Cp[i - 1];
    d.c_z0 = (int64_t)T[i] * h->Cp[i];
    if (!lnx) d.act = DZN_ACT_GELU;
    d.a_amax = s.am(s.conv_slot(cur));   // (r3: the group-norm element pass tracks its |max| too, so conv1 takes the fp16 split)
    if (!lnx) d.c_amax = s.am(s.conv_slot(nxt));
    // (r3) the fused front end also finishes conv1's own LayerNorm + GELU in its epilogue (its tile holds whole rows)
    const bool ln_in_01 = i == 1 && fuse01 && lnx && i != last && h->sw.conv01_ln;
    if (i == 1 && fuse01)
      chk(launch_conv01_fused(wave, B, N, stats, h->conv0_w, h->conv_ln[0].g, h->conv_ln[0].b, h->conv0_lnq, h->C[0],
                              T[0], T[1], h->conv1_W2f, h->conv1_wscf, h->Cp[1], h->conv0_bound, 1e-5f, nxt,
                              st, ln_in_01 ? h->conv_ln[1].g : nullptr, ln_in_01 ? h->conv_ln[1].b : nullptr, h->C[1],
                              ln_in_01 ? s.am(s.conv_slot(nxt)) : nullptr),
          "conv01 fused");
    else
      s.gemm(d, CLS_CONV);
    if (lnx && !ln_in_01)  // channel LayerNorm + GELU (+ dummy_weight after the last conv, components.py:208)
      ln_t(nxt, h->Cp[i], nxt, h->Cp[i], h->conv_ln[i], (int64_t)B * T[i], h->Cp[i], 1, st,
           i == last ? h->dummy_w : nullptr, s.am(s.conv_slot(nxt)), T[i]);
    std::swap(cur, nxt);
  }
  if (!lnx || c.n_conv == 1)
    chk(launch_col_scale(cur, s.ML, h->C[last], h->Cp[last], h->dummy_w, st), "dummy_weight");
  tap(h, "features", cur, s.ML, h->C[last], h->Cp[last], st);
  return cur;
}

// ---- feature projection (components.py:305-306) + positional conv: x = x + gelu(conv_pos(x))  (components.py:980-987,
// 366-380); `feat`: the conv stack's output, in bufA or bufB ----
void seg_project(const SegCall& s, float* feat) {
  H* h = s.h;
  const dzn_config& c = h->cfg;
  hipStream_t st = s.st;
  const int B = s.B, L = s.L, D = h->D;
  const int64_t ML = s.ML;
  {
    // (col_scale of the base model multiplies conv6's output AFTER its tracker: |dummy_weight| ~ 1, and the
    // tracker only needs to bound the magnitude within the 2^15 / 65504 headroom -> skip the fp16 path there)
    const bool tracked = c.extractor_layer_norm && c.n_conv > 1;
    dzn_gemm_desc d = norm_lin_desc(s, h->fp, feat, tracked ? s.conv_slot(feat) : -1, feat == h->bufA ? h->bufB : h->bufA, -1,
                                    h->x, D);
    d.c_amax = s.am(dzn_handle::AM_X);
    s.gemm(d, CLS_FEATPROJ);
  }
  tap(h, "featproj", h->x, ML, D, D, st);

  const bool h2 = prec_is_h2(c.precision);
  const int Kc = c.pos_conv_kernel, G = c.pos_conv_groups, cg = D / G, Lp = L + Kc;
  // f32s: every element of the padded copy feeds 128 taps — split it ONCE here (three bf16 planes) and
  // let the contraction read the planes (gemm_split_pre.hip) instead of re-splitting it per K tile
  const int cgp = h->pos_cgp > 0 ? h->pos_cgp : cg, Dp = G * cgp;     // plane rows: G groups of cgp channels
  const bool pre3 = h->xpad3 != nullptr && (int64_t)c.max_batch * Lp * Dp < (int64_t)1 << 31;
  const bool pre2 = pre3 && h2 && h->posconv.W2h;   // two fp16 planes, scaled by the |max| of x (snapshotted)
  if (pre2)
    chk(launch_pad_rows_split2(h->x, h->xpad3, h->xpad3_plane, B, L, Lp, Kc / 2, Dp, s.am(dzn_handle::AM_X),
                               s.am(dzn_handle::AM_XPAD), st, cg, cgp),
        "pad_rows_split2");
  else if (pre3)
    chk(launch_pad_rows_split3(h->x, h->xpad3, h->xpad3_plane, B, L, Lp, Kc / 2, Dp, st, cg, cgp), "pad_rows_split3");
  else
    chk(launch_pad_rows(h->x, h->xpad, B, L, Lp, Kc / 2, D, st), "pad_rows");
  // the un-split copy (fp32 mode) keeps cg channels per group; the planes have cgp
  const int ca = pre3 ? cgp : cg, Da = pre3 ? Dp : D;
  if (!pre3 && cgp != cg) throw EngineError(DZN_E_INVALID, "padded positional-conv groups need the pre-split planes");
  // one contraction per channel group over ALL B*L rows (row-offset table into the padded copy), so
  // the 128-row tiles are not padded per window (L = 399 would waste 22 % of every window's last tile)
  const bool tabled = (int64_t)c.max_batch * Lp * Da < (int64_t)1 << 31;
  if (tabled) ensure_pos_rowoff(h, L, Lp, Da, st);
  dzn_gemm_desc d = gd(h, h->xpad, h->posconv, h->x, tabled ? ML : L, Da, D);
  d.N = cg;
  d.kc = ca;
  d.ldk = Da;
  d.act = DZN_ACT_GELU;
  d.R = h->x;
  d.a_z1 = ca;
  d.w_z1 = (int64_t)cg * h->posconv.K;
  d.c_z1 = cg;
  d.b_z1 = cg;
  if (tabled) {
    d.a_rowoff = h->pos_rowoff;
    d.nz = G;
    d.zdiv = G;
    d.alg_flops = 2.0 * (double)ML * cg * h->posconv.Kt;
  } else {
    d.nz = B * G;
    d.zdiv = G;
    d.a_z0 = (int64_t)Lp * Da;
    d.c_z0 = (int64_t)L * D;
    d.alg_flops = 2.0 * (double)L * cg * h->posconv.Kt;
  }
  if (pre3) {
    d.A = reinterpret_cast<const float*>(h->xpad3);
    d.a_split3 = pre2 ? 2 : 1;
    d.a_plane = h->xpad3_plane;
    if (pre2) d.a_amax = s.am(dzn_handle::AM_XPAD);
  }
  d.c_amax = s.am(dzn_handle::AM_X);
  // f32h planes of 64 channels per group: the Toeplitz-resident kernel (posconv_resident.hip) when the rows a tile's taps touch
  // fit LDS at this (B, L) — a shape rule like the contraction families' tile rules; everything else keeps the generic kernel
  if (h->posconv_resident && pre2 && tabled && posconv_resident_fits(B, L, Kc)) {
    d.amax_unit = L;
    chk(launch_posconv_resident(d, B, L, Kc, st), "posconv_resident");
  } else {
    s.gemm(d, CLS_POSCONV);
  }
  if (!c.layer_norm_first) ln_t(h->x, D, h->x, D, h->enc_ln, ML, D, 0, st, nullptr, s.am(dzn_handle::AM_X), L);
}

// ---- transformer layer i (components.py:920-942) over the residual stream xr; returns where its output rows live.
// `wsum`: the deferred layer-weighted sum (h->xl), which notes (rows, weight) per layer; else the layer adds its rows to `ws` ----
float* seg_encoder_layer(SegCall& s, int i, float* xr, WsSumArgs& wsum) {
  H* h = s.h;
  hipStream_t st = s.st;
  const int L = s.L, D = h->D;
  const int64_t ML = s.ML;
  const EncLayer& Ly = h->layers[i];
  const bool defer = h->xl != nullptr;
  const float wl = h->wsum_w[i + 1];
  float* const own = defer ? h->xl + (int64_t)i * ML * D : xr;   // where this layer's output rows live
  // the statistics of the rows the next folded LayerNorm reads are already in rstat: left by the previous layer's FFN-down
  // epilogue (an attention-less layer with stats_in), further down by this layer's out_proj epilogue
  bool have_stats = Ly.stats_in && !Ly.attn;
  if (Ly.attn) {
    const int hd = Ly.h * 64;
    // folded LN1: the q/k/v contraction needs the LN statistics and the attention the gate on LN(x), which is never written.
    // stats_in: the previous layer's FFN-down left the rows' partial sums in spart -> gate_heads finishes the statistics and
    // reads the kept heads' channels only; else one pass over the whole rows gives both (gate_stats).
    // Unfolded: the gate reads what the contraction reads.
    const bool gs = Ly.qkv.folded;
    if (gs && Ly.stats_in)
      chk(launch_gate_heads(xr, D, Ly.ln1.g, Ly.ln1.b, Ly.Wg, Ly.bg, Ly.cst, Ly.head_idx, Ly.h, h->spart, s.stat_P, D, 1e-5f,
                            h->gate, h->rstat, ML, h->H, st),
          "gate_heads");
    else if (gs)
      chk(launch_gate_stats(xr, D, Ly.ln1.g, Ly.ln1.b, Ly.Wg, Ly.bg, Ly.cst, h->gate, h->rstat, ML, h->H, 1e-5f, st),
          "gate_stats");
    dzn_gemm_desc d = norm_lin_desc(s, Ly.qkv, xr, dzn_handle::AM_X, h->y, dzn_handle::AM_Y, h->qkv, 3 * hd, gs);
    if (!gs) chk(launch_gate(d.A, D, Ly.Wg, Ly.bg, Ly.cst, h->gate, ML, h->H, st), "gate");
    d.c_amax = s.am(dzn_handle::AM_QKV);
    const bool planes = h->kvp != nullptr && d.W2h && d.col_scale && d.a_amax;     // the f32h contraction writes them
    if (planes) {
      d.kv_planes = h->kvp;
      d.kv_plane_stride = (ML + 64) * (int64_t)(2 * hd);
      d.kv_scale = h->kvs;
      d.kv_ld = 2 * hd;
      d.kv_col0 = hd;
    }
    s.gemm(d, CLS_QKV);
    attention(s, &Ly, h->qkv, dzn_handle::AM_QKV, planes, h->ao);
    dzn_gemm_desc o = gd(h, h->ao, Ly.out, own, ML, hd, D);
    o.R = xr;
    o.a_amax = s.am(dzn_handle::AM_QKV);   // rows of ao are convex combinations of v rows: |ao| <= max |qkv|
    o.c_amax = s.am(dzn_handle::AM_X);
    if (Ly.ffn && Ly.f1.folded && h->sw.epilogue_stats) {
      // the rows it writes are exactly what the FFN's (folded) LayerNorm normalises: leave their statistics
      o.stat_partial = h->spart;
      o.stat_final = h->rstat;
      o.stat_C = D;
      o.stat_eps = 1e-5f;
      have_stats = true;
    }
    s.gemm(o, CLS_OUT);
    xr = own;
  }
  if (!Ly.pre_norm) ln_t(xr, D, xr, D, Ly.ln1, ML, D, 0, st, nullptr, s.am(dzn_handle::AM_X), L);
  if (Ly.ffn) {
    dzn_gemm_desc f1 = norm_lin_desc(s, Ly.f1, xr, dzn_handle::AM_X, h->y, dzn_handle::AM_Y, h->mid, Ly.Fp, have_stats);
    f1.act = DZN_ACT_GELU;
    f1.c_amax = s.am(dzn_handle::AM_MID);
    s.gemm(f1, CLS_FFN1);
    dzn_gemm_desc f2 = gd(h, h->mid, Ly.f2, own, ML, Ly.Fp, D);
    f2.R = xr;
    if (Ly.pre_norm && !defer) {
      f2.WS = h->ws;
      f2.ldws = D;
      f2.ws_w = wl;
    }
    f2.a_amax = s.am(dzn_handle::AM_MID);
    f2.c_amax = s.am(dzn_handle::AM_X);
    const EncLayer* next = i + 1 < h->cfg.n_layers ? &h->layers[i + 1] : nullptr;
    if (next && next->stats_in) {
      // the rows it writes are what the next layer's first (folded) LayerNorm normalises: leave their partial sums.  Before
      // an attention layer nothing finalizes them (stat_final stays null): its gate_heads does, from s.stat_P partials per row
      f2.stat_partial = h->spart;
      f2.stat_final = next->attn ? nullptr : h->rstat;
      f2.stat_C = D;
      f2.stat_eps = 1e-5f;
    }
    s.gemm(f2, CLS_FFN2);
    if (f2.stat_partial) s.stat_P = gemm_stat_partials_last();
    xr = own;
  } else if (Ly.pre_norm && !defer) {
    chk(launch_ws_accum(xr, h->ws, wl, 0, ML * D, st), "ws_accum");
  }
  if (!Ly.pre_norm) {
    ln_t(xr, D, xr, D, Ly.ln2, ML, D, 0, st, nullptr, s.am(dzn_handle::AM_X), L);
    chk(launch_ws_accum(xr, h->ws, wl, 0, ML * D, st), "ws_accum");
  } else if (defer) {   // a layer pruned to nothing leaves xr where it was: the same rows enter the sum again with this weight
    wsum.x[wsum.n] = xr;
    wsum.w[wsum.n++] = wl;
  }
  if (h->sw.debug_taps) {
    const std::string nm = "layer" + std::to_string(i);
    tap(h, nm.c_str(), xr, ML, D, D, st);
  }
  return xr;
}

// ---- head: proj + LN (model_wavlm_conformer.py:256-257) ----
void seg_head_proj(const SegCall& s) {
  H* h = s.h;
  const int A = h->A;
  dzn_gemm_desc d = gd(h, h->ws, h->proj, h->hz, s.ML, h->D, A);
  s.gemm(d, CLS_PROJ);   // (ws has no tracker: bf16 split)
  ln_t(h->hz, A, h->hz, A, h->lnorm, s.ML, A, 0, s.st, nullptr, s.am(dzn_handle::AM_HZ), s.L);
  tap(h, "head_in", h->hz, s.ML, A, A, s.st);
}

// half-step feed-forward of a Conformer layer: hz += 0.5 w2(swish(w1(LN(hz))))
void conf_half_ffn(const SegCall& s, const NormLin& w1, const Lin& w2) {
  H* h = s.h;
  dzn_gemm_desc a = norm_lin_desc(s, w1, h->hz, dzn_handle::AM_HZ, h->ht, -1, h->hmid, h->Fh);
  a.act = DZN_ACT_SWISH;
  a.c_amax = s.am(dzn_handle::AM_HMID);
  s.gemm(a, CLS_CONF_W1);
  dzn_gemm_desc b = gd(h, h->hmid, w2, h->hz, s.ML, h->Fh, h->A);
  b.alpha = 0.5f;
  b.R = h->hz;
  b.a_amax = s.am(dzn_handle::AM_HMID);
  b.c_amax = s.am(dzn_handle::AM_HZ);
  s.gemm(b, CLS_CONF_W2);
}

// ---- Conformer layer i over hz (conformer.py:136-214) ----
void seg_conformer_layer(const SegCall& s, int i) {
  H* h = s.h;
  const dzn_config& c = h->cfg;
  const int A = h->A;
  const int64_t ML = s.ML;
  const ConfLayer& Cl = h->conf[i];
  conf_half_ffn(s, Cl.ffn1_w1, Cl.ffn1_w2);
  {   // MHSA
    dzn_gemm_desc q = norm_lin_desc(s, Cl.qkv, h->hz, dzn_handle::AM_HZ, h->ht, -1, h->hmid, 3 * A);
    q.c_amax = s.am(dzn_handle::AM_HMID);
    s.gemm(q, CLS_CONF_QKV);
    attention(s, nullptr, h->hmid, dzn_handle::AM_HMID, false, h->hv);
    dzn_gemm_desc o = gd(h, h->hv, Cl.o, h->hz, ML, A, A);
    o.R = h->hz;
    o.a_amax = s.am(dzn_handle::AM_HMID);   // attention output <= max |q/k/v| (convex combinations of v)
    o.c_amax = s.am(dzn_handle::AM_HZ);
    s.gemm(o, CLS_CONF_OUT);
  }
  {   // conv module
    dzn_gemm_desc p1 = norm_lin_desc(s, Cl.pw1, h->hz, dzn_handle::AM_HZ, h->ht, -1, h->hmid, 2 * A);
    p1.c_amax = s.am(dzn_handle::AM_HMID);
    s.gemm(p1, CLS_CONF_PW1);
    chk(launch_glu_dwconv(h->hmid, 2 * A, Cl.dw, Cl.dwb, h->hv, A, s.B, s.L, A, c.conf_kernel, s.st), "glu_dwconv");
    dzn_gemm_desc p2 = gd(h, h->hv, Cl.pw2, h->hz, ML, A, A);
    p2.R = h->hz;
    p2.c_amax = s.am(dzn_handle::AM_HZ);    // (glu_dwconv output has no tracker: bf16 split)
    s.gemm(p2, CLS_CONF_PW2);
  }
  conf_half_ffn(s, Cl.ffn2_w1, Cl.ffn2_w2);
  ln_t(h->hz, A, h->hz, A, Cl.out_ln, ML, A, 0, s.st, nullptr, s.am(dzn_handle::AM_HZ), s.L);
  if (h->sw.debug_taps) {
    const std::string nm = "conf" + std::to_string(i);
    tap(h, nm.c_str(), h->hz, ML, A, A, s.st);
  }
}

// the forward of model_wavlm_conformer.py:236-262
void seg_forward(H* h, const float* wave, int B, int N, float* d_logp, uint8_t* d_ml, float* d_soft, hipStream_t st) {
  const dzn_config& c = h->cfg;
  int T[DZN_MAX_CONV];
  {
    int n = N;
    for (int i = 0; i < c.n_conv; ++i) {
      n = conv_out(n, c.conv_k[i], c.conv_s[i]);
      T[i] = n;
    }
  }
  const int L = T[c.n_conv - 1];
  if (L < 1) throw EngineError(DZN_E_INVALID, "window too short");
  const int D = h->D, A = h->A;
  const int64_t ML = (int64_t)B * L, MB = c.max_batch;
  SegCall s{h, st, B, L, ML};
  if (prec_is_h2(c.precision)) {
    chk(launch_fill_u32(h->amax, 0u, dzn_handle::AM_IMG0 * MB, st), "tracker reset");
    if (c.extractor_layer_norm && h->conv0_bound > 0.f) {   // conv0 (LN + GELU) writes bufA: static bound instead of a tracker
      uint32_t bits;
      memcpy(&bits, &h->conv0_bound, 4);
      chk(launch_fill_u32(h->amax + dzn_handle::AM_CONVA * MB, bits, B, st), "conv0 bound");
    }
  }
  seg_project(s, seg_conv_stack(s, wave, N, T));
  // the residual stream: `xr` = rows of the representation the next operation reads.  With the deferred layer-weighted sum
  // every layer moves it into its own buffer (the first residual update of layer i reads xr and writes xl[i], the second
  // one works in place there) and (xr, weight) is noted per layer; else xr == h->x throughout.
  const bool defer = h->xl != nullptr;
  float* xr = h->x;
  WsSumArgs wsum{};
  if (defer) {
    wsum.x[wsum.n] = xr;
    wsum.w[wsum.n++] = h->wsum_w[0];
  } else {
    chk(launch_ws_accum(h->x, h->ws, h->wsum_w[0], 1, ML * D, st), "ws_accum");
  }
  tap(h, "rep0", h->x, ML, D, D, st);
  ensure_table(h, L, st);
  for (int i = 0; i < c.n_layers; ++i) xr = seg_encoder_layer(s, i, xr, wsum);
  if (defer) chk(launch_ws_sum(wsum, h->ws, ML * D, st), "ws_sum");
  tap(h, "wsum", h->ws, ML, D, D, st);
  seg_head_proj(s);
  for (int i = 0; i < c.conf_layers; ++i) seg_conformer_layer(s, i);
  chk(launch_classify(h->hz, A, h->cls_w, h->cls_b, h->mapping, ML, A, c.n_classes,
                      c.max_speakers_per_chunk, d_logp, d_ml, d_soft, st),
      "classify");
}

// ------------------------------------------------------------------ embedding forward
// An image of the trunk with its |max| tracker (null outside the two-term fp16 modes).
struct Img {
  float *p, *am;
};

// What the stages of one emb_forward call share.
struct EmbCall {
  H* h;
  hipStream_t st;
  int B, T, S, L;   // windows, fbank frames per window, masks per window, frames per mask
  // the device-side list of windows with an active speaker (count, ascending list, flag per window): every trunk kernel is
  // launched over all B grid rows with it; all null on the dense path
  const int *z_count, *z_list, *flag;
  // DZN_PREC_F32_H2 / DZN_PREC_F16: one |max| tracker per image buffer (sbuf[stage][k] -> slot AM_IMG0 + 3 stage + k), running
  // over the forward (stem kernel, stage-1 kernel and the contraction epilogues all track what they write)
  float* am(int stage, int k) const {
    return prec_is_h2(h->cfg.precision) ? h->amax + (dzn_handle::AM_IMG0 + 3 * stage + k) * (int64_t)h->cfg.max_batch : nullptr;
  }
  Img image(int stage, int k) const { return {h->sbuf[stage][k], am(stage, k)}; }
};

// one pass of the fbank chain: nsig signals `stride` samples apart, t frames each -> mel energies of their nsig * t
// (<= fb_rows) frames
void fbank_pass(const EmbCall& e, const float* w, int nsig, int64_t stride, int t, float* mel_out) {
  H* h = e.h;
  const int64_t rows = (int64_t)nsig * t;
  chk(launch_frame_prep(w, nsig, stride, t, FB_FLEN, FB_SHIFT, FB_KP, h->hamming, 0.97f, h->frames, e.st), "frame_prep");
  dzn_gemm_desc d = gd(h, h->frames, h->dft, h->spec, rows, FB_KP, 2 * FB_BINS);
  d.precision = DZN_PREC_F32;  // the spectrum spans ~9 decades: keep the transform in fp32
  chk(launch_gemm(d, e.st), "dft");
  chk(launch_power(h->spec, rows, FB_BINS, h->pw, e.st), "power");
  dzn_gemm_desc m = gd(h, h->pw, h->mel, mel_out, rows, FB_BINS, h->cfg.num_mel_bins);
  m.precision = DZN_PREC_F32;
  chk(launch_gemm(m, e.st), "mel");
}

// ---- kaldi fbank + per-window mean subtraction of B windows of N samples into h->fb [B * T, NB] ----
// Window b starts at wave + b * win_stride.  Everything in front of the per-window mean is a function of ONE frame's 400
// samples (DC removal, pre-emphasis, Hamming; the DFT, power and mel contractions are row-independent; the log is per
// element).  When the windows are cut from one recording a whole number q of frame shifts apart (win_stride = 160 q) and
// leave no gap in the frame grid (win_stride <= N - 400 + 160, i.e. q <= T), frame t of window b IS recording frame
// b q + t: the chain runs once over the G = (B - 1) q + T frames of the span the windows cover and log_cmn gathers each
// window's rows.  Any other stride (unrelated windows: win_stride = N) runs the chain per window, read at that stride.
// Either way the chain works in passes of at most fb_rows rows; a row's result does not depend on the pass it is in.
void emb_fbank(const EmbCall& e, const float* wave, int64_t win_stride, int N) {
  H* h = e.h;
  const int B = e.B, T = e.T, NB = h->cfg.num_mel_bins;
  const float eps = 1.1920928955078125e-07f;
  const bool shared = B > 1 && win_stride > 0 && win_stride % FB_SHIFT == 0 && win_stride <= (int64_t)N - FB_FLEN + FB_SHIFT;
  if (shared) {
    const int q = (int)(win_stride / FB_SHIFT);        // <= T, so G <= B * T rows of melg
    const int64_t G = (int64_t)(B - 1) * q + T;
    for (int64_t r0 = 0; r0 < G; r0 += h->fb_rows)
      fbank_pass(e, wave + r0 * FB_SHIFT, 1, 0, (int)std::min<int64_t>(h->fb_rows, G - r0), h->melg + r0 * NB);
    chk(launch_log_cmn_gather(h->melg, q, h->fb, B, T, NB, eps, e.st), "log_cmn");
  } else {
    const int per = (int)std::min<int64_t>(h->fb_rows / T, B);   // fb_rows >= maxTf >= T: at least one window per pass
    for (int b0 = 0; b0 < B; b0 += per)
      fbank_pass(e, wave + b0 * win_stride, std::min(per, B - b0), win_stride, T, h->fb + (int64_t)b0 * T * NB);
    chk(launch_log_cmn(h->fb, B, T, NB, eps, e.st), "log_cmn");
  }
  tap(h, "fbank", h->fb, (int64_t)B * T, NB, NB, e.st);
}

// ---- stem: conv1 + bn1 + relu of the fbank image into buffer 0 of the first stage ----
Img emb_stem(const EmbCall& e) {
  H* h = e.h;
  const Img out = e.image(0, 0);
  chk(launch_stem_conv(h->fb, e.B, e.T, h->cfg.num_mel_bins, h->sC[0], h->stem_w, h->stem_b, out.p, e.st, out.am, e.z_count,
                       e.z_list),
      "stem");
  return out;
}

// the contraction of one ResNet conv over a whole image per window, written to the interior of `out` in this stage
// (tab1): a 3x3 reads patch rows, two-level K = (dh | dw*C + ci); a stride-2 conv reads the previous stage's image (tab2),
// the 1x1 one its centre pixels; windows from the active list; DZN_PREC_F16: two fp16 terms if the trunk's bit asks
dzn_gemm_desc img_desc(const EmbCall& e, const EmbStage& g, const Img& in, const ResConv& rc, const Img& out) {
  const bool down = rc.stride == 2;
  const EmbStage& gin = down ? e.h->stage[g.s - 1] : g;   // the stage whose image it reads (rc.cin planes)
  dzn_gemm_desc d = gd(e.h, rc.ksz == 1 ? in.p + gin.interior : in.p, rc.l, out.p + g.interior, g.M, 0, 0);
  d.a_rowoff = down ? g.tab2 : g.tab1;
  d.c_rowoff = g.tab1;
  if (rc.ksz == 3) {
    d.kc = 3 * rc.cin;
    d.ldk = (int64_t)(gin.Ws + 2) * rc.cin;
  }
  d.nz = e.B;
  d.a_z0 = gin.img;
  d.c_z0 = g.img;
  d.a_amax = in.am;
  d.c_amax = out.am;
  d.z_count = e.z_count;
  d.z_list = e.z_list;
  if (rc.keep2) d.precision = DZN_PREC_F32_H2;
  return d;
}

// a stride-1 3x3 inside stage g.s: out = [relu](act(conv(in)) + R).  x2 (rc.k2 > 0): the previous stage's image, whose centre
// pixels are the second A segment (the folded shortcut)
void conv3(const EmbCall& e, const EmbStage& g, const Img& in, const ResConv& rc, const Img& out, const float* R, int act,
           int post_relu, const Img* x2 = nullptr) {
  if (rc.c32) {
    // first ResNet stage: dedicated kernel, every input pixel split once instead of once per tap
    chk(launch_conv3x3_c32_split(in.p, rc.l.W3, rc.l.b, R, out.p, e.B, g.Hs, g.Ws, act == DZN_ACT_RELU, post_relu, e.st, out.am,
                                 rc.l.W2h, rc.l.wsc, in.am, e.z_count, e.z_list),
        "resnet conv3x3 c32");
    return;
  }
  dzn_gemm_desc d = img_desc(e, g, in, rc, out);
  d.act = act;
  d.R = R ? R + g.interior : nullptr;
  d.post_relu = post_relu;
  if (rc.k2 > 0) {
    d.A2 = x2->p + e.h->stage[g.s - 1].interior;   // pixel (2y, 2x) = centre of conv1's stride-2 patch (rc.k2 planes)
    d.a2_rowoff = g.tab2;
    d.a2_z0 = e.h->stage[g.s - 1].img;
    d.a2_amax = x2->am;
    d.k1 = 9 * rc.cin;
    d.k2 = rc.k2;
  }
  chk(launch_gemm(d, e.st), "resnet conv3x3");
}

// One BasicBlock in the form finalize_emb chose for it.  A stride-1 block reads buffer `cur` of its stage; a down-sampling
// block reads `prev`, the previous stage's output.  Returns the buffer of the stage that holds the block's output.
int emb_block(const EmbCall& e, const EmbStage& g, const ResBlock& rb, const Img& prev, int cur) {
  const int B = e.B, s = g.s;
  const Img in = e.image(s, cur), mid = e.image(s, (cur + 1) % 3), out = e.image(s, (cur + 2) % 3);   // of a stride-1 block
  switch (rb.form) {
    case ResBlock::DOWN:
    case ResBlock::DOWN_FOLDED: {
      // reads the previous stage's image with stride 2 (tab2); buffers 0, 1, 2 = conv1's output, the block's, the shortcut's
      dzn_gemm_desc d = img_desc(e, g, prev, rb.c1, e.image(s, 0));
      d.act = DZN_ACT_RELU;
      chk(launch_gemm(d, e.st), "resnet conv3x3 s2");
      const bool folded = rb.form == ResBlock::DOWN_FOLDED;
      if (!folded) {
        dzn_gemm_desc d1 = img_desc(e, g, prev, rb.sc, e.image(s, 2));
        chk(launch_gemm(d1, e.st), "resnet shortcut");
      }
      // folded: the 1x1 shortcut is k2 more K columns of conv2 (make_resconv_shortcut): no shortcut image, no residual read
      conv3(e, g, e.image(s, 0), rb.c2, e.image(s, 1), folded ? nullptr : e.h->sbuf[s][2], DZN_ACT_NONE, 1, &prev);
      return 1;
    }
    case ResBlock::FUSED32:
      chk(launch_resblock32_fused(in.p, out.p, rb.c1.l.W2h, rb.c1.l.wsc, rb.c1.l.b, rb.c2.l.W2h, rb.c2.l.wsc, rb.c2.l.b, in.am,
                                  out.am, rb.c1.l1max, rb.c1.bmax, B, g.Hs, g.Ws, rb.np, e.st, e.z_count, e.z_list),
          "resblock32 fused");
      break;
    case ResBlock::WS:
      chk(launch_resblock_ws(in.p, out.p, rb.c1.l.W2h, rb.c1.l.wsc, rb.c1.l.b, rb.c2.l.W2h, rb.c2.l.wsc, rb.c2.l.b, in.am, out.am,
                             rb.c1.l1max, rb.c1.bmax, B, g.Hs, g.Ws, rb.c1.cin, e.st, e.z_count, e.z_list, rb.np),
          "resblock ws");
      break;
    case ResBlock::PER_CONV:
      conv3(e, g, in, rb.c1, mid, nullptr, DZN_ACT_RELU, 0);
      conv3(e, g, mid, rb.c2, out, in.p, DZN_ACT_NONE, 1);
  }
  return (cur + 2) % 3;
}

// ---- one stage of the ResNet34 trunk: `prev` = the image it reads (stage 0: the stem's, its own buffer 0; later stages: the
// previous stage's output); returns the image its last block wrote ----
Img emb_stage(const EmbCall& e, int s, const Img& prev) {
  int cur = 0;
  for (const ResBlock& rb : e.h->stages[s]) cur = emb_block(e, e.h->stage[s], rb, prev, cur);
  return e.image(s, cur);
}

// ---- TSTP pooling of the last stage's image `x` for all S masks + seg_1 ----
void emb_pool_head(const EmbCall& e, const Img& x, const float* masks, float* d_emb) {
  H* h = e.h;
  const EmbStage& g = h->stage[3];
  const int feat = g.Cc * g.Hs;
  chk(launch_stats_pool(x.p, e.B, g.Hs, g.Ws, g.Cc, masks, e.S, e.L, h->pool, e.st, e.flag), "stats_pool");
  tap(h, "pool", h->pool, (int64_t)e.B * e.S, 2 * feat, 2 * feat, e.st);
  dzn_gemm_desc d = gd(h, h->pool, h->seg1, d_emb, (int64_t)e.B * e.S, 2 * feat, h->cfg.embed_out_dim);
  d.precision = DZN_PREC_F32;
  chk(launch_gemm(d, e.st), "seg_1");
}

// kaldi fbank -> ResNet34 -> multi-mask TSTP -> seg_1 for B windows of N samples, window b at wave + b * win_stride.
// `subset`: windows in which no speaker is active skip the trunk.  Zero weights pool to zero
// (PA/models/blocks/pooling.py:44-131 with its 1e-8 guards), so every one of their embeddings is seg_1's bias (SURVEY a18;
// tests/test_emb_gpu.py holds the device to that bit for bit).  The masks decide it and they only exist on the device, so
// the subset is built there (window_active -> compact_active: ascending list + count) and every trunk kernel is launched
// over all B grid rows with (count, list): surplus rows exit at once.  No flag is read back — the call only enqueues
// (include/dzn.h), and it can be captured in a HIP graph.  The fbank is computed for every window, silent or not.
void emb_forward(H* h, const float* wave, int64_t win_stride, const float* masks, int B, int S, int N, int L, float* d_emb,
                 hipStream_t st) {
  if (N < FB_FLEN) throw EngineError(DZN_E_INVALID, "waveform shorter than one fbank frame (400 samples)");
  const int T = 1 + (N - FB_FLEN) / FB_SHIFT;
  if (T > h->maxTf) throw EngineError(DZN_E_INVALID, "N exceeds max_samples");
  if (S < 1 || S > 8) throw EngineError(DZN_E_INVALID, "S must be in [1, 8]");
  emb_set_geometry(h, T, st);
  const bool subset = h->sw.emb_skip && !h->sw.debug_taps && h->seg1.b != nullptr;
  const EmbCall e{h, st, B, T, S, L, subset ? h->win_cnt : nullptr, subset ? h->win_idx : nullptr, subset ? h->win_flag : nullptr};
  if (subset) {
    chk(launch_window_active(masks, B, S * L, h->win_flag, st), "window_active");
    chk(launch_compact_active(h->win_flag, B, h->win_cnt, h->win_idx, h->emb_totals, st), "compact_active");
  } else {
    h->emb_dense_windows += B;   // dzn_embed_skip_stats counts every window, whichever path it took
  }
  emb_fbank(e, wave, win_stride, N);
  if (float* am0 = e.am(0, 0)) chk(launch_fill_u32(am0, 0u, 12 * (int64_t)h->cfg.max_batch, st), "image tracker reset");
  Img x = emb_stem(e);
  for (int s = 0; s < 4; ++s) x = emb_stage(e, s, x);
  emb_pool_head(e, x, masks, d_emb);
}

template <typename F>
int guarded(H* h, F&& f) {
  try {
    f();
    return DZN_OK;
  } catch (const EngineError& e) {
    if (h) h->err = e.what();
    else last_create_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    if (h) h->err = "host allocation failed";
    return DZN_E_NOMEM;
  } catch (const std::exception& e) {
    if (h) h->err = e.what();
    return DZN_E_INVALID;
  }
}

}  // namespace

// ====================================================================== C ABI
// conv0's channel-LayerNorm statistics as functions of a frame's k0 samples (frontend.hip): lq[0 .. 10) = wbar = mean over the
// C0 channels of the taps, lq[10 + 10 e + j] = F[e][j] with F^T F = Q = the covariance over channels of the taps; entries of
// taps >= k0 are zero.  Shared by dzn_create and dzn_op_conv0_lnq.
void conv0_lnq_factor(const float* w, int C0, int k0, float* lq) {
  std::vector<double> wb(10, 0.0), Q(100, 0.0);
  for (int ch = 0; ch < C0; ++ch)
    for (int i = 0; i < k0; ++i) wb[i] += (double)w[(size_t)ch * k0 + i] / C0;   // in double: as fp32 the quotient is exact only for C0 = 2^n
  for (int ch = 0; ch < C0; ++ch)
    for (int i = 0; i < k0; ++i)
      for (int j = 0; j < k0; ++j)
        Q[i * 10 + j] += (w[(size_t)ch * k0 + i] - wb[i]) * (w[(size_t)ch * k0 + j] - wb[j]) / C0;
  // var = x^T Q x as a plain sum of products cancels when the frame lies near Q's small-eigenvalue directions (trained
  // DC-blocking / band-pass conv0 taps on low-frequency or quiet audio: ADVICE r2).  Q is PSD: factor it once, in
  // double, as Q = sum_e lambda_e v_e v_e^T (cyclic Jacobi) and ship F[e][j] = sqrt(lambda_e) v_e[j]; the kernels
  // evaluate var = sum_e (F[e] . x)^2 — a sum of squares, nothing to cancel.
  std::vector<double> Aj(Q), V(100, 0.0);
  for (int i = 0; i < 10; ++i) V[i * 10 + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 10; ++p)
      for (int q = p + 1; q < 10; ++q) off += Aj[p * 10 + q] * Aj[p * 10 + q];
    if (off < 1e-300) break;
    for (int p = 0; p < 10; ++p)
      for (int q = p + 1; q < 10; ++q) {
        const double apq = Aj[p * 10 + q];
        if (apq == 0.0) continue;
        const double theta = (Aj[q * 10 + q] - Aj[p * 10 + p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int r = 0; r < 10; ++r) {        // A <- A J (columns p, q)
          const double arp = Aj[r * 10 + p], arq = Aj[r * 10 + q];
          Aj[r * 10 + p] = cs * arp - sn * arq;
          Aj[r * 10 + q] = sn * arp + cs * arq;
        }
        for (int r = 0; r < 10; ++r) {        // A <- J^T A (rows p, q)
          const double apr = Aj[p * 10 + r], aqr = Aj[q * 10 + r];
          Aj[p * 10 + r] = cs * apr - sn * aqr;
          Aj[q * 10 + r] = sn * apr + cs * aqr;
        }
        for (int r = 0; r < 10; ++r) {        // V <- V J
          const double vrp = V[r * 10 + p], vrq = V[r * 10 + q];
          V[r * 10 + p] = cs * vrp - sn * vrq;
          V[r * 10 + q] = sn * vrp + cs * vrq;
        }
      }
  }
  for (int i = 0; i < 110; ++i) lq[i] = 0.f;
  for (int i = 0; i < 10; ++i) lq[i] = (float)wb[i];
  for (int e = 0; e < 10; ++e) {
    const double lam = std::max(Aj[e * 10 + e], 0.0);
    for (int j = 0; j < 10; ++j) lq[10 + e * 10 + j] = (float)(std::sqrt(lam) * V[j * 10 + e]);
  }
}

extern "C" int dzn_op_conv0_lnq(const float* w, int32_t C0, int32_t k, float* lnq110) {
  if (!w || !lnq110 || C0 < 1 || k < 1 || k > 10) return DZN_E_INVALID;
  conv0_lnq_factor(w, C0, k, lnq110);
  return DZN_OK;
}

extern "C" {

int dzn_create(const dzn_config* cfg, dzn_handle** out) {
  if (!cfg || !out) return DZN_E_INVALID;
  if (cfg->struct_size != (int32_t)sizeof(dzn_config)) {
    last_create_error = "dzn_config.struct_size mismatch (ABI)";
    return DZN_E_INVALID;
  }
  if (cfg->precision == DZN_PREC_BF16) {
    last_create_error = "precision 1 (DZN_PREC_BF16) is not an engine mode: the bf16 engine was removed (reduced precision = DZN_PREC_F16)";
    return DZN_E_INVALID;
  }
  if (cfg->max_batch < 1 || cfg->max_samples < 400 ||
      (cfg->precision != DZN_PREC_F32 && cfg->precision != DZN_PREC_F32_SPLIT && cfg->precision != DZN_PREC_F32_H2 &&
       cfg->precision != DZN_PREC_F16)) {
    last_create_error = "bad max_batch / max_samples / precision";
    return DZN_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    last_create_error = "no HIP device visible (libdzn_hip has no CPU fallback)";
    return DZN_E_HIP;
  }
  dzn_handle* h = new (std::nothrow) dzn_handle();
  if (!h) return DZN_E_NOMEM;
  h->cfg = *cfg;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->sw = read_switches();
  *out = h;
  return DZN_OK;
}

int dzn_load_tensor(dzn_handle* h, const char* key, const void* host_ptr, const int64_t* shape,
                    int32_t ndim, int32_t dtype) {
  if (!h || !key || (!host_ptr && ndim > 0) || ndim < 0 || ndim > 8) return DZN_E_INVALID;
  if (h->finalized) {
    h->err = "dzn_load_tensor after dzn_finalize_weights";
    return DZN_E_STATE;
  }
  return guarded(h, [&] {
    HostT t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      if (shape[i] < 0) throw EngineError(DZN_E_INVALID, "negative dimension");
      t.shape.push_back(shape[i]);
      n *= shape[i];
    }
    t.v.resize((size_t)n);
    if (dtype == DZN_F32) {
      memcpy(t.v.data(), host_ptr, (size_t)n * 4);
    } else if (dtype == DZN_F64) {
      const double* p = static_cast<const double*>(host_ptr);
      for (int64_t i = 0; i < n; ++i) t.v[(size_t)i] = (float)p[i];
    } else if (dtype == DZN_I64) {
      const int64_t* p = static_cast<const int64_t*>(host_ptr);
      for (int64_t i = 0; i < n; ++i) t.v[(size_t)i] = (float)p[i];
    } else {
      throw EngineError(DZN_E_INVALID, "unsupported dtype");
    }
    h->sd[key] = std::move(t);
  });
}

int dzn_finalize_weights(dzn_handle* h) {
  if (!h) return DZN_E_INVALID;
  if (h->finalized) {
    h->err = "already finalized";
    return DZN_E_STATE;
  }
  DeviceGuard dg(h->device);
  int rc = guarded(h, [&] {
    h->mx_pack = true;
    finalize_seg(h);
    h->mx_pack = false;
    h->has_emb = h->cfg.has_embedding != 0;
    if (h->has_emb) finalize_emb(h);
    alloc_optional_workspace(h);
    HIPCHK(hipDeviceSynchronize());
  });
  if (rc == DZN_OK) {
    h->finalized = true;
    h->ignored = (int)h->sd.size() - (int)h->used.size();
    h->sd.clear();
  }
  return rc;
}

int dzn_num_frames(const dzn_handle* h, int32_t num_samples) {
  if (!h) return DZN_E_INVALID;
  int n = num_samples;
  for (int i = 0; i < h->cfg.n_conv; ++i) n = conv_out(n, h->cfg.conv_k[i], h->cfg.conv_s[i]);
  return n;
}

int dzn_segment_forward(dzn_handle* h, const float* d_wave, int32_t B, int32_t N, float* d_logp,
                        uint8_t* d_multilabel, void* hip_stream) {
  return dzn_segment_forward_soft(h, d_wave, B, N, d_logp, d_multilabel, nullptr, hip_stream);
}

int dzn_segment_forward_soft(dzn_handle* h, const float* d_wave, int32_t B, int32_t N, float* d_logp,
                             uint8_t* d_multilabel, float* d_soft, void* hip_stream) {
  if (!h) return DZN_E_INVALID;
  if (!h->finalized) {
    h->err = "dzn_segment_forward before dzn_finalize_weights";
    return DZN_E_STATE;
  }
  if (!d_wave || B < 1 || B > h->cfg.max_batch || N > h->cfg.max_samples || N < 1) {
    h->err = "bad B / N (exceeds max_batch / max_samples?)";
    return DZN_E_INVALID;
  }
  DeviceGuard dg(h->device);
  return guarded(h, [&] {
    seg_forward(h, d_wave, B, N, d_logp, d_multilabel, d_soft, reinterpret_cast<hipStream_t>(hip_stream));
  });
}

int dzn_embed_forward(dzn_handle* h, const float* d_wave, const float* d_masks, int32_t B, int32_t S,
                      int32_t N, int32_t L, float* d_emb, void* hip_stream) {
  // dense windows: a stride of N never meets the frame-grid conditions, every window runs its own fbank
  return dzn_embed_forward_strided(h, d_wave, N, d_masks, B, S, N, L, d_emb, hip_stream);
}

int dzn_embed_forward_strided(dzn_handle* h, const float* d_rec, int64_t win_stride, const float* d_masks, int32_t B,
                              int32_t S, int32_t N, int32_t L, float* d_emb, void* hip_stream) {
  if (!h) return DZN_E_INVALID;
  if (!h->finalized || !h->has_emb) {
    h->err = "embedding model not loaded / not finalized";
    return DZN_E_STATE;
  }
  if (!d_rec || !d_masks || !d_emb || B < 1 || B > h->cfg.max_batch || N > h->cfg.max_samples ||
      L < 1 || (B > 1 && win_stride < 0)) {
    h->err = "bad arguments to dzn_embed_forward";
    return DZN_E_INVALID;
  }
  DeviceGuard dg(h->device);
  return guarded(h, [&] {
    emb_forward(h, d_rec, B > 1 ? win_stride : N, d_masks, B, S, N, L, d_emb, reinterpret_cast<hipStream_t>(hip_stream));
  });
}

int dzn_prepare_masks(dzn_handle* h, const uint8_t* d_multilabel, int32_t B, int32_t L,
                      int32_t median_size, int32_t exclude_overlap, int32_t min_num_frames,
                      uint8_t* d_filtered, float* d_masks, void* hip_stream) {
  if (!h || !d_multilabel) return DZN_E_INVALID;
  if (!h->finalized) {
    h->err = "dzn_prepare_masks before dzn_finalize_weights";
    return DZN_E_STATE;
  }
  if (B < 1 || B > h->cfg.max_batch || L < 1 || (!d_filtered && !d_masks)) {
    h->err = "bad arguments to dzn_prepare_masks (B exceeds max_batch?)";
    return DZN_E_INVALID;
  }
  DeviceGuard dg(h->device);
  return guarded(h, [&] {
    chk(launch_prepare_masks(d_multilabel, B, L, h->cfg.max_speakers_per_chunk, median_size,
                             exclude_overlap, min_num_frames, d_filtered, d_masks,
                             reinterpret_cast<hipStream_t>(hip_stream)),
        "prepare_masks");
  });
}

int dzn_debug_fetch(dzn_handle* h, const char* name, float* host_out, int64_t cap, int64_t* n_elems) {
  if (!h || !name) return DZN_E_INVALID;
  auto it = h->taps.find(name);
  if (it == h->taps.end()) {
    h->err = std::string("no such tap (set DZN_DEBUG_TAPS=1 before dzn_create): ") + name;
    return DZN_E_INVALID;
  }
  if (n_elems) *n_elems = (int64_t)it->second.size();
  if (host_out) {
    if (cap < (int64_t)it->second.size()) return DZN_E_INVALID;
    memcpy(host_out, it->second.data(), it->second.size() * 4);
  }
  return DZN_OK;
}

int dzn_embed_skip_stats(const dzn_handle* h, int64_t* windows, int64_t* skipped) {
  if (!h) return DZN_E_INVALID;
  long long t[2] = {0, 0};
  if (h->emb_totals) {      // the totals live on the device (the forward never reads them back): this call synchronises
    DeviceGuard dg(h->device);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(t, h->emb_totals, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess)
      return DZN_E_HIP;
  }
  t[0] += h->emb_dense_windows;
  if (windows) *windows = (int64_t)t[0];
  if (skipped) *skipped = (int64_t)t[1];
  return DZN_OK;
}

int dzn_num_ignored(const dzn_handle* h) { return h ? h->ignored : 0; }
int64_t dzn_workspace_bytes(const dzn_handle* h) { return h ? h->bytes : 0; }

const char* dzn_last_error(const dzn_handle* h) {
  return h ? h->err.c_str() : last_create_error.c_str();
}

int dzn_destroy(dzn_handle* h) {
  if (!h) return DZN_OK;
  DeviceGuard dg(h->device);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return DZN_OK;
}

int dzn_resample(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int32_t channel,
                 int64_t src_first_index, int64_t src_len, int64_t total_len, const float* d_bank, int32_t o, int32_t n,
                 int32_t width, int64_t m0, int64_t m1, float* d_dst, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_resample: " + why;
    return DZN_E_INVALID;
  };
  if (o < 1 || n < 1 || width < 0 || total_len < 0 || src_len < 0 || m0 < 0 || m1 < m0 || !d_bank)
    return refuse("bad o / n / width / lengths / range");
  if (src_format < 0 || src_format >= DZN_SRC_FORMATS || channels < 1)
    return refuse("src_format " + std::to_string(src_format) + " with " + std::to_string(channels) +
                  " channel(s): the formats are 0 (float32 mono) .. 7 (DZN_SRC_* of dzn.h), interleaved over channels >= 1");
  if (src_format == DZN_SRC_F32 && channels != 1)
    return refuse("src_format 0 is float32 mono, not " + std::to_string(channels) +
                  " channels (5 is float32 interleaved over channels)");
  if (channel < DZN_CHANNEL_DOWNMIX || channel >= channels)
    return refuse("channel " + std::to_string(channel) + " of a source with " + std::to_string(channels) + " channel(s)");
  if (total_len > INT64_MAX / n) return refuse("total_len * n overflows");
  if (src_len > INT64_MAX / 4 / channels) return refuse("src_len * channels * bytes per sample overflows");
  const int64_t out_len = (total_len * n + o - 1) / o;
  if (m1 > out_len)
    return refuse("m1 = " + std::to_string(m1) + " is beyond the output length " + std::to_string(out_len));
  if (m1 == m0) return DZN_OK;
  if (!resample_lds_bytes(o, n, width))
    return refuse("o / n = " + std::to_string(o) + " / " + std::to_string(n) + ": the input of one tile does not fit in LDS");
  // what [m0, m1) reads inside the recording
  int64_t lo = (m0 / n) * o - width, hi = ((m1 - 1) / n) * o + width + o;
  lo = lo < 0 ? 0 : lo;
  hi = hi > total_len ? total_len : hi;
  if (lo < hi && (src_first_index > lo || src_first_index + src_len < hi))
    return refuse("the span given, [" + std::to_string(src_first_index) + ", " + std::to_string(src_first_index + src_len) +
                  "), does not cover the input [" + std::to_string(lo) + ", " + std::to_string(hi) + ") that the range reads");
  if (!d_dst || (lo < hi && !d_src)) return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_resample(d_src, src_format, channels, channel, src_first_index, src_len, total_len, d_bank, o, n, width, m0,
                         m1, d_dst, reinterpret_cast<hipStream_t>(hip_stream));
}

int dzn_decode(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int32_t channel, int64_t frames,
               float* d_dst, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_decode: " + why;
    return DZN_E_INVALID;
  };
  if (frames < 0) return refuse("bad frames");
  if (src_format < 0 || src_format >= DZN_SRC_FORMATS || channels < 1)
    return refuse("src_format " + std::to_string(src_format) + " with " + std::to_string(channels) +
                  " channel(s): the formats are 0 (float32 mono) .. 7 (DZN_SRC_* of dzn.h), interleaved over channels >= 1");
  if (src_format == DZN_SRC_F32 && channels != 1)
    return refuse("src_format 0 is float32 mono, not " + std::to_string(channels) +
                  " channels (5 is float32 interleaved over channels)");
  if (channel < DZN_CHANNEL_DOWNMIX || channel >= channels)
    return refuse("channel " + std::to_string(channel) + " of a source with " + std::to_string(channels) + " channel(s)");
  if (frames > INT64_MAX / 4 / channels) return refuse("frames * channels * bytes per sample overflows");
  if (frames == 0) return DZN_OK;
  if (!d_dst || !d_src) return refuse("null pointer");
  const uintptr_t align = src_format == DZN_SRC_S16 ? 2 : (src_format == DZN_SRC_S32 || src_format == DZN_SRC_F32 ||
                                                           src_format == DZN_SRC_F32I) ? 4 : 1;
  if (reinterpret_cast<uintptr_t>(d_src) % align)
    return refuse("d_src is not aligned to the " + std::to_string(align) + "-byte samples of src_format " +
                  std::to_string(src_format));
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_decode(d_src, src_format, channels, channel, frames, d_dst, reinterpret_cast<hipStream_t>(hip_stream));
}

// what dzn_beamform_delays and dzn_beamform_sum refuse alike; "" when the geometry is sound
static std::string beamform_geometry(int32_t channels, int64_t ch_stride, int64_t x_first, int64_t x_len, int64_t T,
                                     int32_t hop) {
  if (channels < 2 || channels > 64)
    return std::to_string(channels) + " channel(s): an array has 2 .. 64";
  if (hop < 256 || hop > 4096 || (hop & (hop - 1)))
    return "hop " + std::to_string(hop) + " is not a power of two in [256, 4096]";
  if (T < 0 || x_len < 0 || x_first < 0 || ch_stride < x_len || T > INT64_MAX / 8 || ch_stride > INT64_MAX / 4 / channels)
    return "bad T / x_first / x_len / ch_stride (ch_stride >= x_len >= 0)";
  return "";
}

static std::string span_text(int64_t lo, int64_t hi) {
  return "[" + std::to_string(lo) + ", " + std::to_string(hi) + ")";
}

int dzn_beamform_delays(int32_t device, const float* d_x, int32_t channels, int64_t ch_stride, int64_t x_first, int64_t x_len,
                        int64_t T, int32_t ref, int32_t hop, int32_t max_lag, const float* d_twiddle, int64_t b0, int64_t b1,
                        int32_t* d_lag, float* d_peak, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_beamform_delays: " + why;
    return DZN_E_INVALID;
  };
  const std::string geo = beamform_geometry(channels, ch_stride, x_first, x_len, T, hop);
  if (!geo.empty()) return refuse(geo);
  if (ref < 0 || ref >= channels)
    return refuse("reference channel " + std::to_string(ref) + " of a source with " + std::to_string(channels) + " channels");
  if (max_lag < 1 || max_lag > hop / 2)
    return refuse("max_lag " + std::to_string(max_lag) + " is outside [1, hop / 2 = " + std::to_string(hop / 2) + "]");
  const int64_t nb = (T + hop - 1) / hop + 1;
  if (b0 < 0 || b1 < b0 || b1 > nb)
    return refuse("blocks " + span_text(b0, b1) + " are not inside the " + std::to_string(nb) + " blocks of the recording");
  if (b1 == b0) return DZN_OK;
  // what frames b0 .. b1 - 1 read inside the recording: samples (b0 - 1) hop .. b1 hop - 1
  int64_t lo = (b0 - 1) * hop, hi = b1 * hop;
  lo = lo < 0 ? 0 : lo;
  hi = hi > T ? T : hi;
  if (lo < hi && (x_first > lo || x_first + x_len < hi))
    return refuse("the span given, " + span_text(x_first, x_first + x_len) + ", does not cover the input " + span_text(lo, hi) +
                  " that the blocks read");
  if (!d_twiddle || !d_lag || !d_peak || (lo < hi && !d_x)) return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_beamform_delays(d_x, channels, ch_stride, x_first, x_len, T, ref, hop, max_lag, d_twiddle, b0, b1, d_lag,
                                d_peak, reinterpret_cast<hipStream_t>(hip_stream));
}

int dzn_beamform_sum(int32_t device, const float* d_x, int32_t channels, int64_t ch_stride, int64_t x_first, int64_t x_len,
                     int64_t T, int32_t hop, const int32_t* d_delay, int64_t num_blocks, int64_t n0, int64_t n1, float* d_dst,
                     void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_beamform_sum: " + why;
    return DZN_E_INVALID;
  };
  const std::string geo = beamform_geometry(channels, ch_stride, x_first, x_len, T, hop);
  if (!geo.empty()) return refuse(geo);
  const int64_t nb = (T + hop - 1) / hop + 1;
  if (num_blocks != nb)
    return refuse("num_blocks = " + std::to_string(num_blocks) + ", a recording of " + std::to_string(T) + " samples has " +
                  std::to_string(nb) + " blocks of hop " + std::to_string(hop));
  if (n0 < 0 || n1 < n0 || n1 > T)
    return refuse("samples " + span_text(n0, n1) + " are not inside the recording of " + std::to_string(T));
  if (n1 == n0) return DZN_OK;
  if (!d_delay || !d_dst) return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  // The delays decide which samples are read, so the columns this range uses — blocks n0 / hop .. (n1 - 1) / hop + 1 of every
  // channel, a few KB — come back to the host and are checked before anything is launched.  This is the one wait of the call:
  // it ends when the stream has produced d_delay.
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const int64_t ba = n0 / hop, bz = (n1 - 1) / hop + 2, cols = bz - ba;
  std::vector<int32_t> dl((size_t)(cols * channels));
  if (hipMemcpy2DAsync(dl.data(), (size_t)cols * 4, d_delay + ba, (size_t)num_blocks * 4, (size_t)cols * 4, (size_t)channels,
                       hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return DZN_E_HIP;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  for (int64_t b = ba; b + 1 < bz; ++b) {      // samples of block b read with the delays of b and b + 1
    const int64_t s0 = n0 > b * hop ? n0 : b * hop, s1 = n1 < (b + 1) * hop ? n1 : (b + 1) * hop;
    for (int32_t c = 0; c < channels; ++c)
      for (int k = 0; k < 2; ++k) {
        const int64_t d = dl[(size_t)(c * cols + (b - ba) + k)];
        if (d < -(hop / 2) || d > hop / 2)
          return refuse("delay " + std::to_string(d) + " of channel " + std::to_string(c) + " in block " +
                        std::to_string(b + k) + " is beyond hop / 2 = " + std::to_string(hop / 2));
        const int64_t a = s0 + d < 0 ? 0 : s0 + d, z = s1 + d > T ? T : s1 + d;
        if (a < z) {
          lo = a < lo ? a : lo;
          hi = z > hi ? z : hi;
        }
      }
  }
  if (lo < hi && (x_first > lo || x_first + x_len < hi))
    return refuse("the span given, " + span_text(x_first, x_first + x_len) + ", does not cover the input " + span_text(lo, hi) +
                  " that the range reads");
  if (lo < hi && !d_x) return refuse("null pointer");
  return launch_beamform_sum(d_x, channels, ch_stride, x_first, x_len, T, hop, d_delay, num_blocks, n0, n1, d_dst, st);
}

// what dzn_decode_planar and dzn_beamform_feed refuse in the stored frames, in dzn_decode's words; "" when they are sound
static std::string planar_source(int32_t src_format, int32_t channels, int64_t frames, int64_t ch_stride, const void* d_src) {
  if (frames < 0) return "bad frames";
  if (src_format < 0 || src_format >= DZN_SRC_FORMATS || channels < 1)
    return "src_format " + std::to_string(src_format) + " with " + std::to_string(channels) +
           " channel(s): the formats are 0 (float32 mono) .. 7 (DZN_SRC_* of dzn.h), interleaved over channels >= 1";
  if (src_format == DZN_SRC_F32 && channels != 1)
    return "src_format 0 is float32 mono, not " + std::to_string(channels) + " channels (5 is float32 interleaved over channels)";
  if (frames > INT64_MAX / 4 / channels) return "frames * channels * bytes per sample overflows";
  if (ch_stride < frames || ch_stride > INT64_MAX / 4 / channels)
    return "ch_stride = " + std::to_string(ch_stride) + " for " + std::to_string(frames) + " frames (ch_stride >= frames)";
  const uintptr_t align = src_format == DZN_SRC_S16 ? 2 : (src_format == DZN_SRC_S32 || src_format == DZN_SRC_F32 ||
                                                           src_format == DZN_SRC_F32I) ? 4 : 1;
  if (reinterpret_cast<uintptr_t>(d_src) % align)
    return "d_src is not aligned to the " + std::to_string(align) + "-byte samples of src_format " + std::to_string(src_format);
  return "";
}

int dzn_decode_planar(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int64_t frames, float* d_dst,
                      int64_t ch_stride, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_decode_planar: " + why;
    return DZN_E_INVALID;
  };
  const std::string bad = planar_source(src_format, channels, frames, ch_stride, d_src);
  if (!bad.empty()) return refuse(bad);
  if (frames == 0) return DZN_OK;
  if (!d_dst || !d_src) return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_decode_planar(d_src, src_format, channels, frames, d_dst, ch_stride, reinterpret_cast<hipStream_t>(hip_stream));
}

// what dzn_beamform_track and dzn_beamform_feed refuse in a block range; "" when it is sound
static std::string track_blocks(int32_t channels, int32_t ref, int32_t hop, int64_t T, int64_t nblk, int64_t b0, int64_t b1,
                                int64_t delay_stride, const int64_t* h_seen) {
  if (channels < 2 || channels > 64) return std::to_string(channels) + " channel(s): an array has 2 .. 64";
  if (ref < 0 || ref >= channels)
    return "reference channel " + std::to_string(ref) + " of a source with " + std::to_string(channels) + " channels";
  if (hop < 256 || hop > 4096 || (hop & (hop - 1))) return "hop " + std::to_string(hop) + " is not a power of two in [256, 4096]";
  if (T < 0 || T > INT64_MAX / 8) return "bad T";
  if (!h_seen) return "null pointer";
  const int64_t nb = (T + hop - 1) / hop + 1;
  if (b0 < 0 || b1 < b0 || b1 > nb)
    return "blocks " + span_text(b0, b1) + " are not inside the " + std::to_string(nb) + " blocks of the recording";
  if (b1 - b0 > nblk || b1 > delay_stride)
    return "blocks " + span_text(b0, b1) + " do not fit lag / peak rows of " + std::to_string(nblk) + " or a delay table of " +
           std::to_string(delay_stride) + " blocks";
  if (b0 != *h_seen)
    return "b0 = " + std::to_string(b0) + " is out of sequence: the state has seen " + std::to_string(*h_seen) + " block(s)";
  return "";
}

int dzn_beamform_track(int32_t device, const int32_t* d_lag, const float* d_peak, int64_t nblk, int32_t channels, int32_t ref,
                       int32_t hop, int64_t T, float min_peak, int64_t b0, int64_t b1, int32_t* d_state, int64_t* h_seen,
                       int32_t* d_delay, int64_t delay_stride, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_beamform_track: " + why;
    return DZN_E_INVALID;
  };
  const std::string bad = track_blocks(channels, ref, hop, T, nblk, b0, b1, delay_stride, h_seen);
  if (!bad.empty()) return refuse(bad);
  if (b1 == b0) return DZN_OK;
  if (!d_lag || !d_peak || !d_state || !d_delay) return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  const int rc = launch_beamform_track(d_lag, d_peak, nblk, channels, ref, hop, T, min_peak, hop / 2, b0, b1, d_state, d_delay,
                                       delay_stride, reinterpret_cast<hipStream_t>(hip_stream));
  if (rc == DZN_OK) *h_seen = b1;
  return rc;
}

// what dzn_beamform_feed and a descriptor of dzn_beamform_many refuse in their arguments; "" when they are sound
static std::string beamform_feed_args(const void* d_src, int32_t src_format, int32_t channels, int64_t src_first,
                                      int64_t src_frames, int64_t T, int32_t ref, int32_t hop, int32_t max_lag, int64_t ch_stride,
                                      int64_t blk_cap, int64_t b0, int64_t b1, const int64_t* h_seen, int64_t table_blocks,
                                      int64_t n0, int64_t n1) {
  std::string bad = planar_source(src_format, channels, src_frames, ch_stride, d_src);
  if (bad.empty()) bad = beamform_geometry(channels, ch_stride, src_first, src_frames, T, hop);
  if (bad.empty() && (max_lag < 1 || max_lag > hop / 2))
    bad = "max_lag " + std::to_string(max_lag) + " is outside [1, hop / 2 = " + std::to_string(hop / 2) + "]";
  if (bad.empty()) bad = track_blocks(channels, ref, hop, T, blk_cap, b0, b1, table_blocks, h_seen);
  if (!bad.empty()) return bad;
  if (n0 < 0 || n1 < n0 || n1 > T)
    return "samples " + span_text(n0, n1) + " are not inside the recording of " + std::to_string(T);
  if (n1 > n0 && (n1 - 1) / hop + 1 >= b1)
    return "samples " + span_text(n0, n1) + " use block " + std::to_string((n1 - 1) / hop + 1) + ", and only the blocks below " +
           std::to_string(b1) + " are tracked after this call";
  // what the call reads inside [0, T): the frames of the blocks, and n + delay with |delay| <= max_lag (the tracker's bound)
  const int64_t x1 = src_first + src_frames;
  if (b1 > b0) {
    int64_t lo = (b0 - 1) * hop, hi = b1 * hop;
    lo = lo < 0 ? 0 : lo;
    hi = hi > T ? T : hi;
    if (lo < hi && (src_first > lo || x1 < hi))
      return "the span given, " + span_text(src_first, x1) + ", does not cover the input " + span_text(lo, hi) +
             " that the blocks read";
  }
  if (n1 > n0) {
    int64_t lo = n0 - max_lag, hi = n1 + max_lag;
    lo = lo < 0 ? 0 : lo;
    hi = hi > T ? T : hi;
    if (lo < hi && (src_first > lo || x1 < hi))
      return "the span given, " + span_text(src_first, x1) + ", does not cover the input " + span_text(lo, hi) +
             " that the samples may read";
  }
  return "";
}

int dzn_beamform_feed(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int64_t src_first,
                      int64_t src_frames, int64_t T, int32_t ref, int32_t hop, int32_t max_lag, float min_peak,
                      const float* d_twiddle, float* d_planar, int64_t ch_stride, int32_t* d_lag, float* d_peak, int64_t blk_cap,
                      int64_t b0, int64_t b1, int32_t* d_state, int64_t* h_seen, int32_t* d_delay, int64_t table_blocks,
                      int64_t n0, int64_t n1, float* d_dst, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_beamform_feed: " + why;
    return DZN_E_INVALID;
  };
  const std::string bad = beamform_feed_args(d_src, src_format, channels, src_first, src_frames, T, ref, hop, max_lag, ch_stride,
                                             blk_cap, b0, b1, h_seen, table_blocks, n0, n1);
  if (!bad.empty()) return refuse(bad);
  if (b1 == b0 && n1 == n0) return DZN_OK;
  if (!d_twiddle || !d_planar || !d_lag || !d_peak || !d_state || !d_delay || (n1 > n0 && !d_dst) || (src_frames > 0 && !d_src))
    return refuse("null pointer");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  int rc = launch_decode_planar(d_src, src_format, channels, src_frames, d_planar, ch_stride, st);
  if (rc != DZN_OK) return rc;
  rc = launch_beamform_delays(d_planar, channels, ch_stride, src_first, src_frames, T, ref, hop, max_lag, d_twiddle, b0, b1,
                              d_lag, d_peak, st);
  if (rc != DZN_OK) return rc;
  rc = launch_beamform_track(d_lag, d_peak, b1 - b0, channels, ref, hop, T, min_peak, max_lag, b0, b1, d_state, d_delay,
                             table_blocks, st);
  if (rc != DZN_OK) return rc;
  *h_seen = b1;
  return launch_beamform_sum(d_planar, channels, ch_stride, src_first, src_frames, T, hop, d_delay, table_blocks, n0, n1, d_dst,
                             st);
}

static_assert(sizeof(dzn_ingest_desc) == 96, "dzn_ingest_desc is 96 bytes without padding (include/dzn.h)");

int dzn_ingest_many(int32_t device, const void* d_stage, int64_t stage_bytes, const dzn_ingest_desc* h_desc,
                    const dzn_ingest_desc* d_desc, int32_t num_desc, const float* d_banks, int64_t bank_floats, float* d_pool,
                    int64_t pool_rows, int64_t row_floats, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_ingest_many: " + why;
    return DZN_E_INVALID;
  };
  if (num_desc < 0 || stage_bytes < 0 || bank_floats < 0 || pool_rows < 0 || row_floats < 0)
    return refuse("bad num_desc / sizes");
  if (num_desc == 0) return DZN_OK;
  if (!h_desc || !d_desc || !d_pool) return refuse("null pointer");
  if (pool_rows && row_floats > INT64_MAX / pool_rows) return refuse("pool_rows * row_floats overflows");
  static const int bytes_of[DZN_SRC_FORMATS] = {4, 2, 1, 3, 4, 4, 1, 1};
  const int64_t tile = dzn_resample_tile();
  int64_t tiles = 0;
  size_t lds = 0;
  double moved = 0.0;
  for (int32_t i = 0; i < num_desc; ++i) {
    const dzn_ingest_desc& d = h_desc[i];
    auto bad = [&](const std::string& why) { return refuse("descriptor " + std::to_string(i) + ": " + why); };
    const bool decode = d.bank_offset < 0;
    if (d.src_format < 0 || d.src_format >= DZN_SRC_FORMATS || d.channels < 1)
      return bad("src_format " + std::to_string(d.src_format) + " with " + std::to_string(d.channels) +
                 " channel(s): the formats are 0 (float32 mono) .. 7 (DZN_SRC_* of dzn.h), interleaved over channels >= 1");
    if (d.src_format == DZN_SRC_F32 && d.channels != 1)
      return bad("src_format 0 is float32 mono, not " + std::to_string(d.channels) + " channels");
    if (d.channel < DZN_CHANNEL_DOWNMIX || d.channel >= d.channels)
      return bad("channel " + std::to_string(d.channel) + " of a source with " + std::to_string(d.channels) + " channel(s)");
    if (d.m0 < 0 || d.m1 < d.m0 || d.src_len < 0 || d.src_offset < 0) return bad("bad lengths / range / offset");
    if (d.src_len > INT64_MAX / 4 / d.channels) return bad("src_len * channels * bytes per sample overflows");
    if (d.tile0 != tiles)
      return bad("tile0 = " + std::to_string(d.tile0) + " is not the tile prefix " + std::to_string(tiles));
    const int64_t count = d.m1 - d.m0;
    // the output range inside ONE pool row
    if (d.dst_offset < 0 || row_floats < 1 || d.dst_offset / row_floats >= pool_rows ||
        d.dst_offset % row_floats + count > row_floats)
      return bad("the output [" + std::to_string(d.dst_offset) + ", " + std::to_string(d.dst_offset + count) +
                 ") reaches past its pool row of " + std::to_string(row_floats) + " floats");
    bool reads = count > 0;
    if (decode) {
      if (d.src_len != count)
        return bad("a decode descriptor holds the " + std::to_string(count) + " frames it decodes, not " +
                   std::to_string(d.src_len));
    } else {
      if (d.o < 1 || d.n < 1 || d.width < 0 || d.total_len < 0) return bad("bad o / n / width / total_len");
      if (d.total_len > INT64_MAX / d.n) return bad("total_len * n overflows");
      const int64_t out_len = (d.total_len * d.n + d.o - 1) / d.o;
      if (d.m1 > out_len) return bad("m1 = " + std::to_string(d.m1) + " is beyond the output length " + std::to_string(out_len));
      if (count > 0) {
        const size_t need = resample_lds_bytes(d.o, d.n, d.width);
        if (!need)
          return bad("o / n = " + std::to_string(d.o) + " / " + std::to_string(d.n) + ": the input of one tile does not fit in LDS");
        lds = need > lds ? need : lds;
        const int64_t K = 2 * (int64_t)d.width + d.o;
        if (!d_banks || d.bank_offset > bank_floats || K * d.n > bank_floats - d.bank_offset)
          return bad("the bank at float " + std::to_string(d.bank_offset) + " leaves the " + std::to_string(bank_floats) +
                     " floats of d_banks");
        int64_t lo = (d.m0 / d.n) * d.o - d.width, hi = ((d.m1 - 1) / d.n) * d.o + d.width + d.o;      // what [m0, m1) reads
        lo = lo < 0 ? 0 : lo;
        hi = hi > d.total_len ? d.total_len : hi;
        reads = lo < hi;
        if (reads && (d.src_first_index > lo || d.src_first_index + d.src_len < hi))
          return bad("the span given, [" + std::to_string(d.src_first_index) + ", " + std::to_string(d.src_first_index + d.src_len) +
                     "), does not cover the input [" + std::to_string(lo) + ", " + std::to_string(hi) + ") that the range reads");
      }
    }
    if (reads) {
      const int64_t nbytes = d.src_len * d.channels * bytes_of[d.src_format];
      if (!d_stage || d.src_offset > stage_bytes || nbytes > stage_bytes - d.src_offset)
        return bad("the source [" + std::to_string(d.src_offset) + ", " + std::to_string(d.src_offset + nbytes) +
                   ") leaves the " + std::to_string(stage_bytes) + " bytes of d_stage");
      const uintptr_t align = d.src_format == DZN_SRC_S16 ? 2 : (d.src_format == DZN_SRC_S32 || d.src_format == DZN_SRC_F32 ||
                                                                 d.src_format == DZN_SRC_F32I) ? 4 : 1;
      if ((reinterpret_cast<uintptr_t>(d_stage) + (uintptr_t)d.src_offset) % align)
        return bad("the source is not aligned to the " + std::to_string(align) + "-byte samples of src_format " +
                   std::to_string(d.src_format));
      moved += (double)nbytes;
    }
    moved += 4.0 * (double)count;
    tiles += (count + tile - 1) / tile;
    if (tiles > 0x7fffffff) return bad("more than 2^31 - 1 tiles");
  }
  if (tiles == 0) return DZN_OK;
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_ingest_many(d_stage, d_desc, num_desc, tiles, lds, moved, d_banks, d_pool,
                            reinterpret_cast<hipStream_t>(hip_stream));
}

static_assert(sizeof(dzn_beamform_desc) == 208, "dzn_beamform_desc is 208 bytes without padding (include/dzn.h)");

int dzn_beamform_many(int32_t device, const void* d_stage, int64_t stage_bytes, const dzn_beamform_desc* h_desc,
                      const dzn_beamform_desc* d_desc, int32_t num_desc, const float* d_twiddles, int64_t twiddle_floats,
                      float* d_planar, int64_t planar_floats, int32_t* d_lag, float* d_peak, int64_t temp_elems,
                      int32_t* d_state, int64_t state_ints, int32_t* d_delay, int64_t delay_ints, float* d_pool,
                      int64_t pool_floats, float* d_beam, int64_t beam_floats, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_beamform_many: " + why;
    return DZN_E_INVALID;
  };
  if (num_desc < 0 || stage_bytes < 0 || twiddle_floats < 0 || planar_floats < 0 || temp_elems < 0 || state_ints < 0 ||
      delay_ints < 0 || pool_floats < 0 || beam_floats < 0)
    return refuse("bad num_desc / sizes");
  if (num_desc == 0) return DZN_OK;
  if (!h_desc || !d_desc) return refuse("null pointer");
  static const int bytes_of[DZN_SRC_FORMATS] = {4, 2, 1, 3, 4, 4, 1, 1};
  const int64_t tile = dzn_beamform_tile();
  // [lo, lo + len) lies inside a buffer of `size` elements (len >= 0)
  auto inside = [](int64_t lo, int64_t len, int64_t size) { return lo >= 0 && len >= 0 && lo <= size && len <= size - lo; };
  auto overlap = [](int64_t a, int64_t al, int64_t b, int64_t bl) { return al > 0 && bl > 0 && a < b + bl && b < a + al; };
  int64_t decode_tiles = 0, gcc_items = 0, sum_tiles = 0;
  int max_hop = 0;
  double work[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // decode bytes, GCC-PHAT flops / bytes, sum flops / bytes
  std::vector<std::array<int64_t, 2>> planars, temps, dsts[2];      // the regions written by the descriptors so far
  bool need[9] = {false, false, false, false, false, false, false, false, false};
  for (int32_t i = 0; i < num_desc; ++i) {
    const dzn_beamform_desc& d = h_desc[i];
    auto bad = [&](const std::string& why) { return refuse("descriptor " + std::to_string(i) + ": " + why); };
    if (d.src_offset < 0 || d.src_offset > stage_bytes) return bad("bad src_offset");
    const void* src = static_cast<const uint8_t*>(d_stage) + d.src_offset;
    const std::string why = beamform_feed_args(src, d.src_format, d.channels, d.src_first, d.src_frames, d.T, d.ref, d.hop,
                                               d.max_lag, d.ch_stride, d.blk_cap, d.b0, d.b1, &d.seen, d.table_blocks, d.n0, d.n1);
    if (!why.empty()) return bad(why);
    if (d.reserved[0] || d.reserved[1] || d.dst_space < 0 || d.dst_space > 1) return bad("bad dst_space / reserved");
    if (d.decode_tile0 != decode_tiles || d.gcc_item0 != gcc_items || d.sum_tile0 != sum_tiles)
      return bad("decode_tile0 / gcc_item0 / sum_tile0 = " + std::to_string(d.decode_tile0) + " / " + std::to_string(d.gcc_item0) +
                 " / " + std::to_string(d.sum_tile0) + " are not the tile prefixes " + std::to_string(decode_tiles) + " / " +
                 std::to_string(gcc_items) + " / " + std::to_string(sum_tiles));
    const int64_t nbytes = d.src_frames * d.channels * bytes_of[d.src_format];
    if (nbytes > 0 && (!d_stage || nbytes > stage_bytes - d.src_offset))
      return bad("the source [" + std::to_string(d.src_offset) + ", " + std::to_string(d.src_offset + nbytes) + ") leaves the " +
                 std::to_string(stage_bytes) + " bytes of d_stage");
    const int64_t nblk = d.b1 - d.b0;
    if (d.s_first < 0 || d.s_first > d.n0) return bad("s_first = " + std::to_string(d.s_first) + " is not in [0, n0]");
    const int64_t hist = d.n0 - d.s_first, count = d.n1 - d.s_first;
    const int64_t plen = (int64_t)d.channels * d.ch_stride, tlen = (int64_t)d.channels * d.blk_cap;
    if (!inside(d.planar_offset, plen, planar_floats))
      return bad("the planar decode at float " + std::to_string(d.planar_offset) + " leaves the " + std::to_string(planar_floats) +
                 " floats of d_planar");
    if (d.blk_cap < 0 || d.blk_cap > INT64_MAX / 64 || !inside(d.lag_offset, tlen, temp_elems))
      return bad("the lag / peak rows at element " + std::to_string(d.lag_offset) + " leave the " + std::to_string(temp_elems) +
                 " elements of d_lag / d_peak");
    if (!inside(d.state_offset, (int64_t)d.channels * DZN_BEAMFORM_STATE_INTS, state_ints))
      return bad("the state at int " + std::to_string(d.state_offset) + " leaves the " + std::to_string(state_ints) +
                 " ints of d_state");
    if (d.table_blocks > INT64_MAX / 4 / d.channels || !inside(d.delay_offset, (int64_t)d.channels * d.table_blocks, delay_ints))
      return bad("the delay table at int " + std::to_string(d.delay_offset) + " leaves the " + std::to_string(delay_ints) +
                 " ints of d_delay");
    if (d.twiddle_offset < 0 || d.twiddle_offset % 2 || !inside(d.twiddle_offset, 2 * (int64_t)d.hop, twiddle_floats))
      return bad("the twiddle table at float " + std::to_string(d.twiddle_offset) + " leaves the " +
                 std::to_string(twiddle_floats) + " floats of d_twiddles");
    if (!inside(d.dst_offset, count, d.dst_space ? beam_floats : pool_floats))
      return bad("the output [" + std::to_string(d.dst_offset) + ", " + std::to_string(d.dst_offset + count) + ") leaves the " +
                 std::to_string(d.dst_space ? beam_floats : pool_floats) + " floats of " + (d.dst_space ? "d_beam" : "d_pool"));
    if (hist > 0) {
      if (!inside(d.carry_offset, hist, beam_floats))
        return bad("the carried samples at float " + std::to_string(d.carry_offset) + " leave the " + std::to_string(beam_floats) +
                   " floats of d_beam");
      if (d.dst_space == 1 && overlap(d.carry_offset, hist, d.dst_offset, count))
        return bad("the carried samples lie in the range the call writes");
    } else if (d.carry_offset < -1) {
      return bad("carry_offset is a float offset or -1");
    }
    for (int32_t j = 0; j < i; ++j) {
      if (h_desc[j].state_offset == d.state_offset)
        return bad("state_offset " + std::to_string(d.state_offset) + " is that of descriptor " + std::to_string(j) +
                   ": two calls of one session never share a table");
      if (overlap(planars[j][0], planars[j][1], d.planar_offset, plen) || overlap(temps[j][0], temps[j][1], d.lag_offset, tlen))
        return bad("its scratch overlaps that of descriptor " + std::to_string(j));
    }
    for (const auto& r : dsts[d.dst_space])
      if (overlap(r[0], r[1], d.dst_offset, count)) return bad("its output overlaps that of an earlier descriptor");
    if (hist > 0)
      for (const auto& r : dsts[1])
        if (overlap(r[0], r[1], d.carry_offset, hist)) return bad("the carried samples lie in the range an earlier descriptor writes");
    planars.push_back({d.planar_offset, plen});
    temps.push_back({d.lag_offset, tlen});
    dsts[d.dst_space].push_back({d.dst_offset, count});
    need[0] |= nbytes > 0;
    need[1] |= nblk > 0;
    need[2] |= count > 0 && d.dst_space == 0;
    need[3] |= (count > 0 && d.dst_space == 1) || hist > 0;
    decode_tiles += (d.src_frames + tile - 1) / tile;
    gcc_items += nblk * (d.channels - 1);
    sum_tiles += (count + tile - 1) / tile;
    if (decode_tiles > 0x7fffffff || gcc_items > 0x7fffffff || sum_tiles > 0x7fffffff) return bad("more than 2^31 - 1 tiles");
    if (nblk > 0 && d.hop > max_hop) max_hop = d.hop;
    int logW = 1;
    while ((1 << logW) < 2 * d.hop) ++logW;
    work[0] += (double)nbytes + 4.0 * (double)d.src_frames * d.channels;
    work[1] += (double)nblk * 2.0 * (d.channels - 1) * 5.0 * 2.0 * d.hop * logW;
    work[2] += (double)nblk * (d.channels - 1) * (16.0 * d.hop + 8.0);
    work[3] += 2.0 * (double)(d.n1 - d.n0) * d.channels;
    work[4] += 4.0 * (double)(d.n1 - d.n0) * (d.channels + 1) + 8.0 * (double)hist;
  }
  if ((need[0] && !d_planar) || (need[1] && (!d_twiddles || !d_planar || !d_lag || !d_peak || !d_state || !d_delay)) ||
      (need[2] && (!d_pool || !d_delay || !d_planar)) || (need[3] && (!d_beam || !d_delay || !d_planar)))
    return refuse("null pointer");
  if (decode_tiles == 0 && gcc_items == 0 && sum_tiles == 0) return DZN_OK;
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_beamform_many(d_stage, d_desc, num_desc, decode_tiles, gcc_items, sum_tiles, max_hop, work, d_twiddles,
                              d_planar, d_lag, d_peak, d_state, d_delay, d_pool, d_beam, reinterpret_cast<hipStream_t>(hip_stream));
}

int dzn_gather_windows(int32_t device, const float* d_pool, int64_t pool_floats, const int64_t* h_offsets,
                       const int64_t* d_offsets, int32_t B, int32_t window, float* d_dst, void* hip_stream) {
  auto refuse = [](const std::string& why) {
    last_create_error = "dzn_gather_windows: " + why;
    return DZN_E_INVALID;
  };
  if (B < 0 || B > 65535 || window < 1 || pool_floats < 0) return refuse("bad B (0 .. 65535) / window / pool_floats");
  if (B == 0) return DZN_OK;
  if (!d_pool || !h_offsets || !d_offsets || !d_dst) return refuse("null pointer");
  for (int32_t b = 0; b < B; ++b)
    if (h_offsets[b] < 0 || h_offsets[b] > pool_floats - window)
      return refuse("window " + std::to_string(b) + " at float " + std::to_string(h_offsets[b]) + " leaves the pool of " +
                    std::to_string(pool_floats) + " floats");
  DeviceGuard dg(device);
  if (!dg.ok) return DZN_E_HIP;
  return launch_gather_windows(d_pool, d_offsets, B, window, d_dst, reinterpret_cast<hipStream_t>(hip_stream));
}

const char* dzn_version(void) {
#ifdef DZN_CHECKED
  return "dzn-hip 0.3.0 (gfx950, MFMA f32 / fp16x2 / bf16x3 / fp16 + MX fp8) [checked build: device-side bounds assertions]";
#else
  return "dzn-hip 0.3.0 (gfx950, MFMA f32 / fp16x2 / bf16x3 / fp16 + MX fp8)";
#endif
}

// CHECKED builds (csrc/checked.h): failed device-side checks of every translation unit since the last reset.
// out4 = {failed checks, id of the first, its workgroup, its detail value}; returns the number of failed checks, 0 in a clean
// run, DZN_E_STATE when the library is not a checked build.
#ifdef DZN_CHECKED
extern "C" {
int dzn_checked_collect_gemm_split(unsigned int*, int);
int dzn_checked_collect_gemm_mx(unsigned int*, int);
int dzn_checked_collect_gemm_split_pre(unsigned int*, int);
int dzn_checked_collect_resblock_fused(unsigned int*, int);
int dzn_checked_collect_resblock_ws(unsigned int*, int);
int dzn_checked_collect_attention_split(unsigned int*, int);
int dzn_checked_collect_attention_planes(unsigned int*, int);
int dzn_checked_collect_frontend_fused(unsigned int*, int);
int dzn_checked_collect_post(unsigned int*, int);
int dzn_checked_collect_resample(unsigned int*, int);
int dzn_checked_collect_ingest(unsigned int*, int);
int dzn_checked_collect_gallery(unsigned int*, int);
int dzn_checked_collect_beamform(unsigned int*, int);
int dzn_checked_collect_beamform_live(unsigned int*, int);
int dzn_checked_collect_beamform_many(unsigned int*, int);
}
#endif
int dzn_checked_status(uint32_t* out4, int32_t reset) {
#ifdef DZN_CHECKED
  typedef int (*collect_fn)(unsigned int*, int);
  const collect_fn fns[] = {dzn_checked_collect_gemm_split, dzn_checked_collect_gemm_mx, dzn_checked_collect_gemm_split_pre,
                            dzn_checked_collect_resblock_fused, dzn_checked_collect_resblock_ws,
                            dzn_checked_collect_attention_split, dzn_checked_collect_attention_planes,
                            dzn_checked_collect_frontend_fused, dzn_checked_collect_post,
                            dzn_checked_collect_resample, dzn_checked_collect_ingest, dzn_checked_collect_gallery,
                            dzn_checked_collect_beamform, dzn_checked_collect_beamform_live,
                            dzn_checked_collect_beamform_many};
  unsigned int tot[4] = {0u, 0u, 0u, 0u};
  for (collect_fn f : fns) {
    unsigned int w[4] = {0u, 0u, 0u, 0u};
    if (f(w, reset) != 0) return DZN_E_HIP;
    if (w[0] && !tot[0]) { tot[1] = w[1]; tot[2] = w[2]; tot[3] = w[3]; }
    tot[0] += w[0];
  }
  if (out4) for (int i = 0; i < 4; ++i) out4[i] = tot[i];
  return (int)tot[0];
#else
  (void)out4;
  (void)reset;
  return DZN_E_STATE;
#endif
}

int dzn_op_relpos_bucket(int32_t rel, int32_t num_buckets, int32_t max_distance) {
  return relpos_bucket(rel, num_buckets, max_distance);
}

}  // extern "C"
