// post.hip — on-device glue between the two device stages, so a window never leaves HBM between
// segmentation and embedding:
//   * median filter along frames of the hard multilabel decisions
//     (diarizen/pipelines/inference.py:131-132: scipy.ndimage.median_filter(size=(1,11,1),
//      mode="reflect"); on {0,1} data the median of an odd window is a majority vote);
//   * embedding masks (PA/pipelines/speaker_diarization.py:268-322): frames with >= 2 active
//     speakers are zeroed ("clean" mask); a speaker falls back to its full mask when its clean
//     mask has <= min_num_frames frames.
// Integer/byte work, one workgroup per window, everything staged in LDS.
// Also the two detection pipelines' aggregation and hysteresis (dzn_detect, below) and the aggregation of the soft scores
// into per-speaker activity scores (dzn_speaker_scores).
#include "common.h"
#include "checked.h"

DZN_CHECKED_TU(post)

namespace {

__global__ __launch_bounds__(256) void prepare_masks_kernel(const uint8_t* __restrict__ ml, int L, int S,
                                                            int median, int exclude_overlap,
                                                            int min_num_frames,
                                                            uint8_t* __restrict__ filtered,
                                                            float* __restrict__ masks) {
  extern __shared__ unsigned char sm[];
  unsigned char* raw = sm;                 // [L*S]
  unsigned char* fil = sm + L * S;         // [L*S]
  int* cnt = reinterpret_cast<int*>(sm + 2 * ((L * S + 3) & ~3));  // [S] clean-frame counts
  const int b = blockIdx.x;
  const uint8_t* in = ml + (int64_t)b * L * S;
  for (int i = threadIdx.x; i < L * S; i += 256) raw[i] = in[i];
  if (threadIdx.x < S) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int half = median / 2;
  for (int i = threadIdx.x; i < L * S; i += 256) {
    const int t = i / S, s = i - t * S;
    unsigned char v = raw[i];
    if (median > 1) {
      int ones = 0;
      for (int d = -half; d <= half; ++d) {
        // scipy 'reflect' (d c b a | a b c d | d c b a) has period 2L: a window longer than the signal reflects again
        int tt = t + d;
        if (tt < 0 || tt >= L) {
          const int m = ((tt % (2 * L)) + 2 * L) % (2 * L);
          tt = m < L ? m : 2 * L - 1 - m;
        }
        ones += raw[tt * S + s];
      }
      v = ones > half ? 1 : 0;
    }
    fil[i] = v;
  }
  __syncthreads();
  if (filtered) {
    uint8_t* out = filtered + (int64_t)b * L * S;
    for (int i = threadIdx.x; i < L * S; i += 256) out[i] = fil[i];
  }
  if (!masks) return;
  // clean-frame counts per speaker
  for (int t = threadIdx.x; t < L; t += 256) {
    int act = 0;
    for (int s = 0; s < S; ++s) act += fil[t * S + s];
    if (act < 2)
      for (int s = 0; s < S; ++s)
        if (fil[t * S + s]) atomicAdd(&cnt[s], 1);
  }
  __syncthreads();
  float* mo = masks + (int64_t)b * S * L;
  for (int i = threadIdx.x; i < L * S; i += 256) {
    const int s = i / L, t = i - s * L;
    int act = 0;
    for (int k = 0; k < S; ++k) act += fil[t * S + k];
    const unsigned char full = fil[t * S + s];
    const bool use_clean = exclude_overlap && cnt[s] > min_num_frames;
    mo[i] = (use_clean ? (act < 2 ? full : 0) : full) ? 1.0f : 0.0f;
  }
}

// ---- host post-processing moved to the device -------------------------------------------
// Inference.aggregate (PA/core/inference.py:574-666) for the two uses of the pipeline — speaker counting
// (PA/pipelines/utils/diarization.py:147-155) and reconstruct / to_diarization (PA/pipelines/speaker_diarization.py:
// 400-425, diarization.py:213-239) — is an overlap-add of small integers: window c adds its L frames at
// start_frame[c] (host-computed with the reference's float64 closest_frame, so no float semantics live here).
// Integer atomics: order independent, bit-reproducible.
__global__ __launch_bounds__(256) void count_accum_kernel(const uint8_t* __restrict__ seg, int64_t CL, int L, int S,
                                                          const int32_t* __restrict__ start, int T,
                                                          int32_t* __restrict__ sum, int32_t* __restrict__ cnt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < CL; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / L), l = (int)(i - (int64_t)c * L);
    const int t = start[c] + l;
    if (t < 0 || t >= T) continue;
    int tot = 0;
    for (int s = 0; s < S; ++s) tot += seg[i * S + s];
    if (tot) atomicAdd(sum + t, tot);
    atomicAdd(cnt + t, 1);
  }
}

// count[t] = uint8(rint(sum / max(cnt, 1e-12))) in float32 like the reference's float32 accumulators; frames no
// window covers are `missing = 0`
__global__ __launch_bounds__(256) void count_finalize_kernel(const int32_t* __restrict__ sum, const int32_t* __restrict__ cnt,
                                                             int T, uint8_t* __restrict__ count) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const float avg = cnt[t] ? __fdiv_rn((float)sum[t], fmaxf((float)cnt[t], 1e-12f)) : 0.f;
  count[t] = (uint8_t)rintf(avg);
}

// act[t, k] += max_s { seg[c, l, s] : hard[c, s] == k }   (skip_average=True; clusters absent from a window are NaN in
// the reference = contribute nothing)
__global__ __launch_bounds__(256) void cluster_accum_kernel(const uint8_t* __restrict__ seg, const int8_t* __restrict__ hard,
                                                            int64_t CL, int L, int S, const int32_t* __restrict__ start,
                                                            int T, int K, int32_t* __restrict__ act) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < CL; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / L), l = (int)(i - (int64_t)c * L);
    const int t = start[c] + l;
    if (t < 0 || t >= T) continue;
    unsigned mask = 0;
    for (int s = 0; s < S; ++s) {
      const int k = hard[c * S + s];
      if (k >= 0 && k < K && seg[i * S + s]) mask |= 1u << k;
    }
    while (mask) {
      const int k = __ffs(mask) - 1;
      mask &= mask - 1;
      atomicAdd(act + (int64_t)t * K + k, 1);
    }
  }
}


// ---- voice activity / overlapped speech detection (dzn_detect) --------------------------------------------------------
// Inference.aggregate(hamming=True, missing=0.0, warm_up) (PA/core/inference.py:389-397, 544-666) of the pre-aggregation
// hooks max_s (voice_activity_detection.py:125) and second-largest_s (overlapped_speech_detection.py:132) over hard 0/1
// decisions.  The reference adds window after window into float32 arrays with float64 operands:
//     acc[t] = f32(f64(acc[t]) + score * mask * hamming[l] * warm_up[l]),   cnt[t] likewise without the score,
// so the rounding sequence is the window order.  One thread per output frame walks ITS covering windows in ascending order
// (start[] is non-decreasing: closest_frame of increasing times) and reproduces that sequence; the file is compiled with
// -ffp-contract=off, and the float64 adds are spelled __dadd_rn so no contraction can creep in.  score * mask is 0 or 1, so the
// float64 product is the host's weight table w[l] = hamming[l] * warm_up[l] (the same two factors, the same product) or 0.
// The kernel computes frames [t0, t1) into rows t - t0 (dzn_detect: t0 = 0; dzn_detect_range: the frames a new window
// changed): a frame's walk depends on nothing but t, so a range is the same bits as the same rows of the whole.
__global__ __launch_bounds__(256) void detect_scores_kernel(const uint8_t* __restrict__ seg, int C, int L, int S,
                                                            const int32_t* __restrict__ start, const double* __restrict__ w,
                                                            int t0, int t1, int tasks, int K, float* __restrict__ scores) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= t1 - t0) return;
  const int t = t0 + row;
  DZN_CHECK(row >= 0 && t >= t0 && t < t1, 0x804, row);
  // covering windows: start[c] <= t < start[c] + L  ->  c in [c0, c1)
  int lo = 0, hi = C;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] > t - L) hi = mid; else lo = mid + 1;
  }
  const int c0 = lo;
  hi = C;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] > t) hi = mid; else lo = mid + 1;
  }
  const int c1 = lo;
  float sp = 0.f, ov = 0.f, cnt = 0.f;
  for (int c = c0; c < c1; ++c) {
    const int l = t - start[c];
    DZN_CHECK(l >= 0 && l < L, 0x800, c);
    DZN_CHECK(c == 0 || start[c - 1] <= start[c], 0x801, c);
    if (l < 0 || l >= L) continue;          // only reachable with a start[] that is not non-decreasing
    const uint8_t* row = seg + ((int64_t)c * L + l) * S;
    int act = 0;
    for (int s = 0; s < S; ++s) act += row[s] != 0;
    const double wl = w[l];
    sp = (float)__dadd_rn((double)sp, act >= 1 ? wl : 0.0);
    ov = (float)__dadd_rn((double)ov, act >= 2 ? wl : 0.0);
    cnt = (float)__dadd_rn((double)cnt, wl);
  }
  // average = acc / max(cnt, epsilon) in float32 (count_finalize_kernel); frames no window covers are `missing` = 0
  const float den = fmaxf(cnt, 1e-12f);
  float* out = scores + (int64_t)row * K;
  int k = 0;
  if (tasks & 1) out[k++] = c1 > c0 ? __fdiv_rn(sp, den) : 0.f;
  if (tasks & 2) out[k++] = c1 > c0 ? __fdiv_rn(ov, den) : 0.f;
  DZN_CHECK(k == K, 0x802, k);
}

// Binarize's hysteresis (PA/utils/signal.py:270-296) as a scan.  Frame t >= 1 is DECISIVE when y > onset (-> active) or
// y < offset (-> inactive); with onset >= offset the two cannot both hold and the reference's state machine is "the verdict
// of the last decisive frame", frame 0 always deciding (y[0] > onset).  Comparisons in float32 against float32 thresholds:
// the reference compares numpy float32 scalars with Python floats, which numpy >= 2 (NEP 50) evaluates in float32.
// One workgroup per task column; each thread owns a contiguous chunk, chunk summaries (-1 = no decisive frame) are combined
// by a Hillis-Steele scan in LDS (right-most defined value wins), then every thread re-walks its chunk from its entry state.
// The scan runs over the n frames [t0, t0 + n) held in rows 0 .. n of scores / active.  Only GLOBAL frame 0 decides
// unconditionally; for t0 > 0 the state before the first decisive frame of the range is entry[k], the state of frame
// t0 - 1 (a range with no decisive frame keeps it throughout).
constexpr int kHystThreads = 1024;

__global__ __launch_bounds__(kHystThreads) void hysteresis_kernel(const float* __restrict__ scores, int t0, int n, int K,
                                                                  float onset, float offset,
                                                                  const uint8_t* __restrict__ entry,
                                                                  uint8_t* __restrict__ active) {
  __shared__ int8_t sv[kHystThreads];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int per = (n + kHystThreads - 1) / kHystThreads;
  const int r0 = min(tid * per, n), r1 = min(r0 + per, n);
  int v = -1;
  for (int r = r0; r < r1; ++r) {
    const float y = scores[(int64_t)r * K + k];
    if (t0 + r == 0) v = y > onset;
    else if (y > onset) v = 1;
    else if (y < offset) v = 0;
  }
  sv[tid] = (int8_t)v;
  __syncthreads();
  for (int off = 1; off < kHystThreads; off <<= 1) {
    const int8_t mine = sv[tid], left = tid >= off ? sv[tid - off] : (int8_t)-1;
    __syncthreads();
    sv[tid] = mine >= 0 ? mine : left;
    __syncthreads();
  }
  // entry state of this chunk: the last decisive frame to its left in the range, else the caller's (t0 > 0); with t0 == 0
  // frame 0 is decisive, so every later chunk finds one and thread 0 needs none
  int state = tid > 0 ? sv[tid - 1] : -1;
  if (state < 0 && t0 > 0) {
    DZN_CHECK(entry[k] <= 1, 0x805, entry[k]);
    state = entry[k] != 0;
  }
  DZN_CHECK(r0 == r1 || (t0 == 0 && tid == 0) || state >= 0, 0x803, tid);
  for (int r = r0; r < r1; ++r) {
    const float y = scores[(int64_t)r * K + k];
    if (t0 + r == 0) state = y > onset;
    else if (y > onset) state = 1;
    else if (y < offset) state = 0;
    DZN_CHECK(r >= 0 && r < n && state >= 0, 0x806, r);
    active[(int64_t)r * K + k] = (uint8_t)state;
  }
}

// ---- per-speaker activity scores (dzn_speaker_scores) -----------------------------------------------------------------
// SpeakerDiarization.reconstruct's clustered scores (PA/pipelines/speaker_diarization.py:400-423: max over the local
// speakers of window c that belong to cluster k, NaN when there is none, hard < 0 skipped) through
// Inference.aggregate(hamming=True, missing=0.0, skip_average=False, warm_up) (PA/core/inference.py:544-666).  The clustered
// array is float64 holding float32 values and every window is added as
//     acc[t,k] = f32(f64(acc[t,k]) + ((score * mask) * hamming[l]) * warm_up[l]),   cnt[t,k] likewise with mask alone
// (mask = 0 and score = 0 for a NaN entry: both additions are of 0.0).  As in detect_scores_kernel one thread — here per
// (t, k) — walks ITS covering windows in ascending order, so the rounding sequence is the reference's; the products and sums
// are spelled __dmul_rn / __dadd_rn (no contraction), and the two weight tables stay apart because the score is not 0 / 1.
__global__ __launch_bounds__(256) void speaker_scores_kernel(const float* __restrict__ soft, const int8_t* __restrict__ hard,
                                                             int C, int L, int S, const int32_t* __restrict__ start,
                                                             const double* __restrict__ ham, const double* __restrict__ wu,
                                                             int T, int K, float* __restrict__ scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)T * K) return;
  const int t = (int)(i / K), k = (int)(i - (int64_t)t * K);
  DZN_CHECK(t >= 0 && t < T && k >= 0 && k < K, 0x812, t);
  // covering windows: start[c] <= t < start[c] + L  ->  c in [c0, c1)
  int lo = 0, hi = C;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] > t - L) hi = mid; else lo = mid + 1;
  }
  const int c0 = lo;
  hi = C;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] > t) hi = mid; else lo = mid + 1;
  }
  const int c1 = lo;
  float acc = 0.f, cnt = 0.f;
  bool seen = false;
  for (int c = c0; c < c1; ++c) {
    const int l = t - start[c];
    DZN_CHECK(l >= 0 && l < L, 0x810, c);
    DZN_CHECK(c == 0 || start[c - 1] <= start[c], 0x811, c);
    if (l < 0 || l >= L) continue;          // only reachable with a start[] that is not non-decreasing
    const float* row = soft + ((int64_t)c * L + l) * S;
    const int8_t* hc = hard + (int64_t)c * S;
    bool has = false, isnan_ = false;
    float v = 0.f;
    for (int s = 0; s < S; ++s) {
      if (hc[s] != k) continue;
      const float x = row[s];
      isnan_ |= x != x;                         // np.max propagates a NaN: the entry is then missing like an absent cluster
      v = (!has || x > v) ? x : v;
      has = true;
    }
    const bool valid = has && !isnan_;
    const double sc = valid ? (double)v : 0.0, m = valid ? 1.0 : 0.0;
    const double hl = ham[l], wl = wu[l];
    acc = (float)__dadd_rn((double)acc, __dmul_rn(__dmul_rn(__dmul_rn(sc, m), hl), wl));
    cnt = (float)__dadd_rn((double)cnt, __dmul_rn(__dmul_rn(m, hl), wl));
    seen |= valid;
  }
  // average = acc / max(cnt, epsilon) in float32; `missing` = 0 where no non-NaN entry landed
  scores[i] = seen ? __fdiv_rn(acc, fmaxf(cnt, 1e-12f)) : 0.f;
}

// ---- live diarization: count -> reconstruct -> top-count over a frame range (dzn_diarize_range) ------------------------
// The chain count_accum/count_finalize -> cluster_accum -> to_diarization's selection (PA/pipelines/utils/diarization.py:
// 121-157, 213-236; PA/pipelines/speaker_diarization.py:400-425) for frames [t0, t1) into rows t - t0.  As in
// detect_scores_kernel a frame's walk over ITS covering windows depends on nothing but t, so a range is the same bytes as the
// same rows of the whole, and there is nothing to zero and nothing to add atomically.  A workgroup holds 256 >> kp_log2 frames
// of KP = 1 << kp_log2 >= K lanes each; lane (f, k) adds up act[t, k] — and, the row of decisions being in its registers
// anyway, the frame's total of active local speakers, so every lane of a frame knows count[t] without an exchange.  The K
// activations of a frame then meet in LDS and lane k takes its rank among them,
//     rank = #{j : act_j > act_k or (act_j == act_k and j < k)},
// which is k's position in np.argsort(-act, kind="stable"); it is active when rank < min(count, K).  KP is a power of two
// <= 32, so a frame never straddles a wave64 and the lanes of a frame read one LDS address (a broadcast).
//
// SCORES (dzn_diarize_range_scores): lane (f, k) is also the thread speaker_scores_kernel would run for (t, k) — the same windows
// in the same ascending order, hard[c, :] already at hand — so the score walk joins the loop with that kernel's arithmetic, term
// for term: the float32 max over the local speakers of label k (a NaN or no speaker: a missing entry that adds two zeros),
// ((score * mask) * hamming[l]) * warm_up[l] in __dmul_rn / __dadd_rn into float32 accumulators, one __fdiv_rn at the end.  The
// accumulators are registers of the lane: no LDS beyond the ranking's, nothing atomic, and the u8 / int32 outputs are computed
// by the very statements of the plain form.
template <bool SCORES>
__global__ __launch_bounds__(256) void diarize_range_kernel(const uint8_t* __restrict__ seg, const int8_t* __restrict__ hard,
                                                            const float* __restrict__ soft, int C, int L, int S,
                                                            const int32_t* __restrict__ start, const double* __restrict__ ham,
                                                            const double* __restrict__ wu, int t0, int t1, int K, int kp_log2,
                                                            int max_count, uint8_t* __restrict__ count,
                                                            uint8_t* __restrict__ active, int32_t* __restrict__ act_out,
                                                            float* __restrict__ scores) {
  __shared__ int32_t sa[256];
  const int tid = threadIdx.x;
  const int f = tid >> kp_log2, k = tid & ((1 << kp_log2) - 1);
  const int64_t row = (int64_t)blockIdx.x * (256 >> kp_log2) + f;
  const bool live = row < (int64_t)(t1 - t0) && k < K;
  const int t = t0 + (int)(live ? row : 0);
  int a = 0, tot = 0, cover = 0;
  float acc = 0.f, wsum = 0.f;
  bool seen = false;
  if (live) {
    // covering windows: start[c] <= t < start[c] + L  ->  c in [c0, c1)
    int lo = 0, hi = C;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start[mid] > t - L) hi = mid; else lo = mid + 1;
    }
    const int c0 = lo;
    hi = C;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int c1 = lo;
    for (int c = c0; c < c1; ++c) {
      const int l = t - start[c];
      DZN_CHECK(l >= 0 && l < L, 0x830, c);
      DZN_CHECK(c == 0 || start[c - 1] <= start[c], 0x831, c);
      if (l < 0 || l >= L) continue;          // only reachable with a start[] that is not non-decreasing
      const uint8_t* r = seg + ((int64_t)c * L + l) * S;
      const int8_t* hc = hard + (int64_t)c * S;
      int v = 0;
      for (int s = 0; s < S; ++s) {
        const int x = r[s];
        tot += x;
        if (hc[s] == k) v = x > v ? x : v;      // k >= 0: an inactive local speaker (hard < 0) matches no lane
      }
      a += v;
      ++cover;
      if (SCORES) {
        DZN_CHECK((int64_t)c * L + l < (int64_t)C * L, 0x833, c);
        const float* fr = soft + ((int64_t)c * L + l) * S;
        bool has = false, isnan_ = false;
        float fv = 0.f;
        for (int s = 0; s < S; ++s) {
          if (hc[s] != k) continue;
          const float x = fr[s];
          isnan_ |= x != x;                       // np.max propagates a NaN: the entry is then missing like an absent label
          fv = (!has || x > fv) ? x : fv;
          has = true;
        }
        const bool valid = has && !isnan_;
        const double sc = valid ? (double)fv : 0.0, m = valid ? 1.0 : 0.0;
        const double hl = ham[l], wl = wu[l];
        acc = (float)__dadd_rn((double)acc, __dmul_rn(__dmul_rn(__dmul_rn(sc, m), hl), wl));
        wsum = (float)__dadd_rn((double)wsum, __dmul_rn(__dmul_rn(m, hl), wl));
        seen |= valid;
      }
    }
  }
  sa[tid] = a;
  __syncthreads();
  if (!live) return;
  // count_finalize_kernel's arithmetic, then the cap (count.data = np.minimum(count.data, max_speakers))
  const float avg = cover ? __fdiv_rn((float)tot, fmaxf((float)cover, 1e-12f)) : 0.f;
  const int cnt = min((int)(uint8_t)rintf(avg), max_count);
  const int32_t* fa = sa + (f << kp_log2);
  int rank = 0;
  for (int j = 0; j < K; ++j) {
    const int aj = fa[j];
    rank += (aj > a || (aj == a && j < k)) ? 1 : 0;
  }
  DZN_CHECK(row >= 0 && row < t1 - t0 && rank < K, 0x832, (int)row);
  if (k == 0) count[row] = (uint8_t)cnt;
  active[row * K + k] = rank < min(cnt, K) ? 1 : 0;
  if (act_out) act_out[row * K + k] = a;
  if (SCORES) {
    DZN_CHECK(row * K + k < (int64_t)(t1 - t0) * K, 0x834, (int)row);
    // average = acc / max(weight sum, epsilon) in float32; `missing` = 0 where no non-NaN entry landed
    scores[row * K + k] = seen ? __fdiv_rn(acc, fmaxf(wsum, 1e-12f)) : 0.f;
  }
}

// the one launch behind dzn_diarize_range (d_scores == nullptr: the plain form) and dzn_diarize_range_scores
int launch_diarize_range(const uint8_t* d_seg, const int8_t* d_hard, const float* d_soft, int C, int L, int S,
                         const int32_t* d_start_frame, const double* d_hamming, const double* d_warm_up, int t0, int t1, int K,
                         int max_count, uint8_t* d_count, uint8_t* d_active, int32_t* d_act, float* d_scores, void* stream) {
  if (!d_seg || !d_hard || !d_start_frame || !d_count || !d_active || C < 0 || L < 1 || S < 1 || S > 8 || t0 < 0 || t1 < t0 ||
      K < 1 || K > 32 || max_count < 0)
    return DZN_E_INVALID;
  if (t1 == t0) return DZN_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int kp_log2 = 0;
  while ((1 << kp_log2) < K) ++kp_log2;         // lanes per frame: the power of two >= K (<= 32)
  const int per_block = 256 >> kp_log2;
  const int n = t1 - t0;
  hipLaunchKernelGGL(d_scores ? diarize_range_kernel<true> : diarize_range_kernel<false>, dim3((unsigned)cdiv64(n, per_block)),
                     dim3(256), 0, st, d_seg, d_hard, d_soft, C, L, S, d_start_frame, d_hamming, d_warm_up, t0, t1, K, kp_log2,
                     max_count, d_count, d_active, d_act, d_scores);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

}  // namespace

extern "C" int dzn_diarize_range(const uint8_t* d_seg, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                                 const int32_t* d_start_frame, int32_t t0, int32_t t1, int32_t K, int32_t max_count,
                                 uint8_t* d_count, uint8_t* d_active, int32_t* d_act, void* stream) {
  return launch_diarize_range(d_seg, d_hard, nullptr, C, L, S, d_start_frame, nullptr, nullptr, t0, t1, K, max_count, d_count,
                              d_active, d_act, nullptr, stream);
}

// the same launch with the per-speaker activity scores of the same frames (dzn_speaker_scores' bits) as a fourth output
extern "C" int dzn_diarize_range_scores(const uint8_t* d_seg, const int8_t* d_hard, const float* d_soft, int32_t C, int32_t L,
                                        int32_t S, const int32_t* d_start_frame, const double* d_hamming,
                                        const double* d_warm_up, int32_t t0, int32_t t1, int32_t K, int32_t max_count,
                                        uint8_t* d_count, uint8_t* d_active, int32_t* d_act, float* d_scores, void* stream) {
  if (!d_soft || !d_hamming || !d_warm_up || !d_scores) return DZN_E_INVALID;
  return launch_diarize_range(d_seg, d_hard, d_soft, C, L, S, d_start_frame, d_hamming, d_warm_up, t0, t1, K, max_count,
                              d_count, d_active, d_act, d_scores, stream);
}

extern "C" int dzn_speaker_count(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame,
                                 int32_t T, int32_t* d_work, uint8_t* d_count, void* stream) {
  if (!d_seg || !d_start_frame || !d_work || !d_count || C < 0 || L < 1 || S < 1 || T < 1) return DZN_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(d_work, 0, sizeof(int32_t) * 2 * (size_t)T, st) != hipSuccess) return DZN_E_HIP;
  const int64_t CL = (int64_t)C * L;
  if (CL > 0) {
    int64_t g = cdiv64(CL, 256);
    g = g > 8192 ? 8192 : g;
    hipLaunchKernelGGL(count_accum_kernel, dim3((unsigned)g), dim3(256), 0, st, d_seg, CL, L, S, d_start_frame, T,
                       d_work, d_work + T);
  }
  hipLaunchKernelGGL(count_finalize_kernel, dim3((T + 255) / 256), dim3(256), 0, st, d_work, d_work + T, T, d_count);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_cluster_activations(const uint8_t* d_seg, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                                       const int32_t* d_start_frame, int32_t T, int32_t K, int32_t* d_act, void* stream) {
  if (!d_seg || !d_hard || !d_start_frame || !d_act || C < 0 || L < 1 || S < 1 || T < 1 || K < 1 || K > 32)
    return DZN_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(d_act, 0, sizeof(int32_t) * (size_t)T * K, st) != hipSuccess) return DZN_E_HIP;
  const int64_t CL = (int64_t)C * L;
  if (CL > 0) {
    int64_t g = cdiv64(CL, 256);
    g = g > 8192 ? 8192 : g;
    hipLaunchKernelGGL(cluster_accum_kernel, dim3((unsigned)g), dim3(256), 0, st, d_seg, d_hard, CL, L, S, d_start_frame,
                       T, K, d_act);
  }
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

extern "C" int dzn_detect_range(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame,
                                const double* d_weight, int32_t t0, int32_t t1, int32_t tasks, float onset, float offset,
                                const uint8_t* d_entry, float* d_scores, uint8_t* d_active, void* stream) {
  if (!d_seg || !d_start_frame || !d_weight || !d_scores || C < 0 || L < 1 || S < 1 || S > 8 || t0 < 0 || t1 < t0 ||
      (tasks & 3) == 0 || (tasks & ~3) != 0 || !(offset <= onset) || (t0 > 0 && !d_entry))
    return DZN_E_INVALID;
  if (t1 == t0) return DZN_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int K = (tasks & 1) + ((tasks >> 1) & 1);
  const int n = t1 - t0;
  hipLaunchKernelGGL(detect_scores_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_seg, C, L, S, d_start_frame, d_weight, t0,
                     t1, tasks, K, d_scores);
  if (d_active)
    hipLaunchKernelGGL(hysteresis_kernel, dim3(K), dim3(kHystThreads), 0, st, d_scores, t0, n, K, onset, offset, d_entry,
                       d_active);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

// the whole recording is the range [0, T) with no entry state
extern "C" int dzn_detect(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame,
                          const double* d_weight, int32_t T, int32_t tasks, float onset, float offset, float* d_scores,
                          uint8_t* d_active, void* stream) {
  if (T < 1) return DZN_E_INVALID;
  return dzn_detect_range(d_seg, C, L, S, d_start_frame, d_weight, 0, T, tasks, onset, offset, nullptr, d_scores, d_active,
                          stream);
}

extern "C" int dzn_speaker_scores(const float* d_soft, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                                  const int32_t* d_start_frame, const double* d_hamming, const double* d_warm_up,
                                  int32_t T, int32_t K, float* d_scores, void* stream) {
  if (!d_soft || !d_hard || !d_start_frame || !d_hamming || !d_warm_up || !d_scores || C < 0 || L < 1 || S < 1 || S > 8 ||
      T < 1 || K < 1 || K > 32)
    return DZN_E_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)T * K;
  hipLaunchKernelGGL(speaker_scores_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, d_soft, d_hard, C, L, S,
                     d_start_frame, d_hamming, d_warm_up, T, K, d_scores);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}

int launch_prepare_masks(const uint8_t* ml, int B, int L, int S, int median, int exclude_overlap,
                         int min_num_frames, uint8_t* filtered, float* masks, hipStream_t st) {
  ProfScope prof_scope_(st, "prepare_masks", 0.0, (double)B * L * S * (2.0 + 4.0));
  if (B <= 0) return DZN_OK;
  if (S < 1 || S > 8 || L < 1 || (median > 1 && !(median & 1))) return DZN_E_INVALID;
  const size_t lds = 2 * (((size_t)L * S + 3) & ~(size_t)3) + 8 * sizeof(int);
  if (lds > 64 * 1024) return DZN_E_INVALID;
  hipLaunchKernelGGL(prepare_masks_kernel, dim3(B), dim3(256), lds, st, ml, L, S, median,
                     exclude_overlap, min_num_frames, filtered, masks);
  return hipGetLastError() == hipSuccess ? DZN_OK : DZN_E_HIP;
}
