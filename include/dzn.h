/*
 * dzn.h — C ABI of libdzn_hip.so, the MI355X (gfx950) engine for the DiariZen
 * sliding-window inference hot path.
 *
 * Plain C, no torch types: every buffer is a raw pointer + sizes.  The caller owns
 * all I/O buffers (for PyTorch-ROCm these are tensor.data_ptr()); the library owns
 * weights and workspace.  All entry points return 0 on success or a negative
 * DZN_E_* code; the message is available through dzn_last_error().  Nothing throws
 * across the boundary.
 *
 * What each entry point replaces in the reference (paths relative to the
 * BUTSpeechFIT/DiariZen tree, PA/ = pyannote-audio/pyannote/audio/):
 *
 *   dzn_create + dzn_load_tensor + dzn_finalize_weights
 *       <- PA/core/model.py:360-369   instantiate(config["model"]["path"], args) ;
 *                                      model.load_state_dict(torch.load(ckpt))
 *          diarizen/models/eend/model_wavlm_conformer.py:26-76 (Model.__init__)
 *          PA/models/embedding/wespeaker/__init__.py:207-233 (WeSpeakerResNet34)
 *   dzn_segment_forward
 *       <- PA/core/inference.py:215       self.model(chunks.to(device))
 *          diarizen/models/eend/model_wavlm_conformer.py:238-264 (Model.forward)
 *          PA/core/inference.py:226 + PA/utils/powerset.py:103-128
 *                                      (Powerset.to_multilabel, soft=False)
 *   dzn_embed_forward
 *       <- PA/pipelines/speaker_verification.py:693-705 (embedding __call__)
 *          PA/models/embedding/wespeaker/__init__.py:190-204 (fbank -> resnet)
 *          PA/models/embedding/wespeaker/resnet.py:344-376 ; PA/models/blocks/pooling.py:44-131
 *   dzn_destroy            <- python object lifetime
 *
 * Threading: one handle per device; calls on one handle are not re-entrant.  Calls
 * only ENQUEUE work on the given HIP stream; the caller synchronises (matching the
 * reference's single-threaded, one-stream use).  One exception, once per geometry: the
 * FIRST forward at a new window length builds that length's index tables (relative-position
 * bias table, positional-conv and ResNet row-offset tables) with synchronous uploads; every
 * later call at that length enqueues only — dzn_segment_forward -> dzn_prepare_masks ->
 * dzn_embed_forward can then be captured in a HIP graph and replayed (r4:
 * tests/test_emb_gpu.py::test_forwards_only_enqueue_and_replay_from_a_hip_graph).
 */
#ifndef DZN_H_
#define DZN_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DZN_MAX_CONV 8
#define DZN_MAX_LAYERS 32
#define DZN_MAX_HEADS 16

#define DZN_OK 0
#define DZN_E_INVALID (-1)   /* bad argument / shape / config                  */
#define DZN_E_NOMEM (-2)     /* device or host allocation failed (-> MemoryError, PA/core/inference.py:216-221) */
#define DZN_E_HIP (-3)       /* HIP runtime error                              */
#define DZN_E_STATE (-4)     /* call order violated (e.g. forward before finalize) */
#define DZN_E_MISSING (-5)   /* a required state_dict key was never loaded     */

/* element types accepted by dzn_load_tensor */
#define DZN_F32 0
#define DZN_F64 1
#define DZN_I64 2

/* arithmetic of the MFMA contractions */
#define DZN_PREC_F32 0   /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 everywhere          */
#define DZN_PREC_BF16 1  /* reserved: no engine mode and no kernel (dzn_create and dzn_op_gemm refuse it with DZN_E_INVALID) */
#define DZN_PREC_F32_SPLIT 2 /* fp32 data everywhere; contractions split both operands exactly into
                                3 bf16 terms and run 6 bf16 MFMA products with fp32 accumulate
                                (fp32-grade accuracy, csrc/gemm_split.hip) */
#define DZN_PREC_F32_H2 3 /* fp32 data everywhere; contractions split both operands into TWO fp16 terms
                           * (exact power-of-two scaling, 22 significant bits) and sum three
                           * v_mfma_f32_16x16x32_f16 products in fp32 ("3xFP16", the error-corrected scheme
                           * known from 3xTF32): csrc/gemm_split.hip NP = 2.  Kernels without an fp16
                           * variant run as DZN_PREC_F32_SPLIT. */
#define DZN_PREC_F16 4 /* REDUCED precision (BASELINE configs[4] "fp16"): the DZN_PREC_F32_H2 engine with the
                        * linear-layer / positional-conv / ResNet contractions keeping only the LEADING fp16 term
                        * of both operands (one v_mfma_f32_16x16x32_f16 product, fp32 accumulate; the same
                        * per-window power-of-two scaling, so no fp16 range issue).  Attention, the fused
                        * conv0->conv1 frontend and the 32-channel 3x3 convolutions keep two terms; data,
                        * norms, softmax and the residual stream stay fp32.  Tolerance class: the bf16 one. */

/*
 * Architecture description.  Mirrors the kwargs of
 * diarizen/models/module/wav2vec2/model.py:779-913 (wavlm_model) as listed in
 * diarizen/models/module/wavlm_config.py, plus Model.__init__ of
 * diarizen/models/eend/model_wavlm_conformer.py:26-45.
 */
typedef struct dzn_config {
  int32_t struct_size;         /* sizeof(dzn_config), ABI check */
  int32_t precision;           /* DZN_PREC_* */
  int32_t max_batch;           /* largest B passed to *_forward */
  int32_t max_samples;         /* largest N (samples per window) */

  /* ---- WavLM frontend ---- */
  int32_t extractor_layer_norm;   /* 1: extractor_mode="layer_norm" (large), 0: "group_norm" (base) */
  int32_t normalize_waveform;     /* W2V/model.py:113 */
  int32_t n_conv;
  int32_t conv_ch[DZN_MAX_CONV];
  int32_t conv_k[DZN_MAX_CONV];
  int32_t conv_s[DZN_MAX_CONV];

  /* ---- WavLM encoder ---- */
  int32_t embed_dim;
  int32_t total_heads;
  int32_t n_layers;
  int32_t layer_norm_first;       /* encoder_layer_norm_first */
  int32_t pos_conv_kernel;
  int32_t pos_conv_groups;
  int32_t num_buckets;
  int32_t max_distance;
  int32_t use_attention[DZN_MAX_LAYERS];
  int32_t n_heads[DZN_MAX_LAYERS];                       /* len(remaining_heads[i]) */
  int32_t head_idx[DZN_MAX_LAYERS][DZN_MAX_HEADS];       /* remaining_heads[i][j]   */
  int32_t use_ffn[DZN_MAX_LAYERS];
  int32_t ffn_dim[DZN_MAX_LAYERS];

  /* ---- EEND Conformer head ---- */
  int32_t attention_in;           /* 256 */
  int32_t ffn_hidden;             /* 1024 */
  int32_t conf_heads;             /* 4 */
  int32_t conf_layers;            /* 4 */
  int32_t conf_kernel;            /* 31 */
  int32_t n_classes;              /* 11 powerset classes */
  int32_t max_speakers_per_chunk; /* 4 */
  int32_t max_speakers_per_frame; /* 2 */

  /* ---- WeSpeaker ResNet34 embedding ---- */
  int32_t has_embedding;          /* 0: segmentation only */
  int32_t embed_out_dim;          /* 256 */
  int32_t num_mel_bins;           /* 80 */
  int32_t reserved[16];
} dzn_config;

typedef struct dzn_handle dzn_handle;

/* Create an engine on the current HIP device.
 * Workspace (allocated when the weights are finalised, sized for max_batch windows of max_samples): besides the activation
 * buffers, pre-norm (layer_norm_first) encoders in the fp32 modes take n_layers further [max_batch * frames, D] fp32 buffers —
 * every layer's output rows stay in the layer's own buffer and the layer-weighted sum (model_wavlm_conformer.py:236,253-254)
 * is one pass over them after the last layer instead of a read-modify-write per layer (same additions, same order, same bits;
 * 22.6 GB at 576 windows of 8 s for wavlm-large).  They are taken only while they fit in half of the free device memory;
 * DZN_NO_WS_DEFER in the environment at that time keeps the per-layer read-modify-write. */
int dzn_create(const dzn_config* cfg, dzn_handle** out);

/*
 * Hand one state_dict entry to the engine (host memory, copied before return).
 * Keys are the reference's own:  segmentation keys as saved from Model
 * ("wavlm_model.feature_extractor.conv_layers.0.conv.weight", ..., "classifier.bias"),
 * embedding keys prefixed "embedding." + the WeSpeakerResNet34 key
 * ("embedding.resnet.conv1.weight", ...).  Unknown keys are ignored
 * (load_state_dict(strict=False) semantics) but counted; see dzn_num_ignored().
 */
int dzn_load_tensor(dzn_handle* h, const char* key, const void* host_ptr,
                    const int64_t* shape, int32_t ndim, int32_t dtype);

/* Fold weight-norm / BatchNorm / dummy_weight, pack + pad for MFMA tiles, upload,
 * allocate workspace for (max_batch, max_samples). */
int dzn_finalize_weights(dzn_handle* h);

/* number of frames L for N samples (model_wavlm_conformer.py:98-124) */
int dzn_num_frames(const dzn_handle* h, int32_t num_samples);

/*
 * Segmentation forward.  d_wave: device f32 [B, N] (channel already selected,
 * inference.py:128 / model_wavlm_conformer.py:250).  Outputs (device, either may
 * be NULL): d_logp f32 [B, L, n_classes] log-probabilities; d_multilabel u8
 * [B, L, max_speakers_per_chunk] hard multilabel decisions.
 *
 * Window isolation (this call, its _soft form and both embedding forwards): a window's results depend on that window's
 * samples and masks alone — not on B, on the window's place in the batch, on max_batch / max_samples or on what the handle
 * ran before — also when another window of the batch or an earlier call on the handle held non-finite samples (NaN, Inf,
 * values whose square overflows).  What the non-finite window itself returns is unspecified.
 */
int dzn_segment_forward(dzn_handle* h, const float* d_wave, int32_t B, int32_t N,
                        float* d_logp, uint8_t* d_multilabel, void* hip_stream);

/*
 * Segmentation forward with the soft multilabel scores as a third optional output: d_soft f32
 * [B, L, max_speakers_per_chunk] (may be NULL: then this is dzn_segment_forward),
 *     soft[b, l, s] = sum over the powerset classes c that contain speaker s, in ascending c, of expf(logp[b, l, c])
 * i.e. Powerset.to_multilabel(powerset, soft=True) = exp(powerset) @ mapping (PA/utils/powerset.py:103-128), the soft
 * path the reference carries through SpeakerDiarization.get_segmentations(file, soft=...)
 * (PA/pipelines/speaker_diarization.py:209-226) and Inference.__call__ / slide / infer (PA/core/inference.py:197-226,
 * 242, 319, 330, 412-444).  Written by the classifier's own launch from the log-probabilities it holds in registers.
 * Enqueue-only, every precision mode.
 */
int dzn_segment_forward_soft(dzn_handle* h, const float* d_wave, int32_t B, int32_t N,
                             float* d_logp, uint8_t* d_multilabel, float* d_soft, void* hip_stream);

/*
 * Embedding forward with the ResNet trunk shared by the S masks of a window.
 * d_wave f32 [B, N]; d_masks f32 [B, S, L]; d_emb f32 [B, S, embed_out_dim].
 */
int dzn_embed_forward(dzn_handle* h, const float* d_wave, const float* d_masks,
                      int32_t B, int32_t S, int32_t N, int32_t L, float* d_emb,
                      void* hip_stream);

/*
 * The same forward over windows cut from ONE recording: window b is the N samples at d_rec + b * win_stride, all of
 * them inside one allocation (the caller's strided view of the recording; no dense copy of the windows is needed).
 * Same results, bit for bit, as dzn_embed_forward on the dense copy of those windows.
 *
 * kaldi's fbank frames are 400 samples long and 160 apart, and everything in front of the per-window mean subtraction
 * is a function of one frame alone.  When
 *     win_stride % 160 == 0   and   0 < win_stride <= N - 400 + 160
 * (windows a whole number q = win_stride / 160 of frames apart, leaving no gap in the frame grid), frame t of window b
 * is recording frame b q + t: framing, DFT, power and mel contraction then run ONCE over the (B - 1) q + T frames the
 * windows cover instead of over B * T rows (windows a tenth of their length apart share 90 % of them).  Any other
 * stride is served by the per-window arithmetic of dzn_embed_forward, reading the windows at their stride; it is not
 * an error.  win_stride is ignored for B == 1.  Enqueue-only and capturable like every forward: no read-back, no
 * allocation, no second stream.
 */
int dzn_embed_forward_strided(dzn_handle* h, const float* d_rec, int64_t win_stride, const float* d_masks,
                              int32_t B, int32_t S, int32_t N, int32_t L, float* d_emb,
                              void* hip_stream);

/*
 * On-device glue between the two stages (keeps a window in HBM):
 *   median filter (odd `median_size`, 0/1 = off) along frames of d_multilabel u8 [B, L, S]
 *       <- diarizen/pipelines/inference.py:131-132 (scipy median_filter size=(1,11,1), "reflect")
 *   embedding masks f32 [B, S, L]: overlap excluded, fallback to the full mask when the clean
 *   mask has <= min_num_frames frames
 *       <- PA/pipelines/speaker_diarization.py:268-322
 * d_filtered u8 [B, L, S] (may be NULL) receives the filtered decisions, d_masks may be NULL.
 */
int dzn_prepare_masks(dzn_handle* h, const uint8_t* d_multilabel, int32_t B, int32_t L,
                      int32_t median_size, int32_t exclude_overlap, int32_t min_num_frames,
                      uint8_t* d_filtered, float* d_masks, void* hip_stream);

/*
 * Host post-processing on the device (stateless, no handle): the two overlap-add aggregations of
 * the pipeline over the per-window decisions that are already in HBM.
 *   dzn_speaker_count       <- SpeakerDiarizationMixin.speaker_count + Inference.aggregate(hamming=False,
 *                              skip_average=False, missing=0)   PA/pipelines/utils/diarization.py:147-155,
 *                              PA/core/inference.py:574-666:  count[t] = uint8(rint(sum_c sum_s seg / #windows))
 *   dzn_cluster_activations <- SpeakerDiarization.reconstruct + the aggregate(skip_average=True) of to_diarization
 *                              PA/pipelines/speaker_diarization.py:400-425, diarization.py:213-220:
 *                              act[t,k] = sum_c max_s{seg[c,t-start_c,s] : hard[c,s]==k}   (hard < 0 = inactive)
 * d_seg u8 [C,L,S]; d_start_frame int32 [C] = closest_frame(c*step + duration_frame/2) computed by the caller with
 * the reference's float64 arithmetic; T = number of output frames.  d_work int32 [2T] scratch; d_act int32 [T,K], K<=32.
 */
int dzn_speaker_count(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame, int32_t T,
                      int32_t* d_work, uint8_t* d_count, void* hip_stream);
int dzn_cluster_activations(const uint8_t* d_seg, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                            const int32_t* d_start_frame, int32_t T, int32_t K, int32_t* d_act, void* hip_stream);

/*
 * Voice activity / overlapped speech detection from the per-window decisions (stateless, no handle; the detection pipelines
 * of diarizen_amd/detection.py):
 *   scores  <- Inference.aggregate(hamming=True, missing=0.0, warm_up) of the pre-aggregation hook
 *              PA/core/inference.py:389-403, 544-666 with
 *              bit 0 (speech)  np.max(scores, axis=-1)                     PA/pipelines/voice_activity_detection.py:125
 *              bit 1 (overlap) np.partition(scores, -2, axis=-1)[..., -2]   PA/pipelines/overlapped_speech_detection.py:132
 *   active  <- Binarize's hysteresis (onset, offset; strict > / <, frames at a threshold keep the state)
 *              PA/utils/signal.py:254-296
 * d_seg u8 [C,L,S] hard decisions (S <= 8), d_start_frame int32 [C] non-decreasing (closest_frame, host float64, as for
 * dzn_speaker_count), d_weight f64 [L] = np.hamming(L) * warm-up window (host), T = output frames (the cropped length:
 * frames >= T are not computed).  `tasks` selects the columns of d_scores f32 [T,K] / d_active u8 [T,K] in bit order
 * (K = number of bits set).  d_active may be NULL (scores only).  The float64 accumulation order is the reference's window
 * order, so the scores are the reference's bits.  Thresholds are float32; offset <= onset.
 */
int dzn_detect(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame, const double* d_weight,
               int32_t T, int32_t tasks, float onset, float offset, float* d_scores, uint8_t* d_active, void* hip_stream);

/*
 * The range form of dzn_detect, for a recording that is still arriving (diarizen_amd/detection.py, DetectionStream): frames
 * [t0, t1) only, into rows t - t0 of d_scores f32 [t1-t0, K] / d_active u8 [t1-t0, K] (may be NULL).
 *   scores  the same per-frame walk over the windows d_start_frame[0..C) that cover t, in ascending window order
 *           (Inference.aggregate, PA/core/inference.py:544-666): a frame's score depends on t and on those windows only, so
 *           it is final once every window covering it is among the C — every t < the start frame of window C
 *   active  Binarize's hysteresis (PA/utils/signal.py:254-296) continued across calls: "frame 0 decides by y > onset" holds
 *           for global frame 0 only; for t0 > 0, d_entry u8 [K] is the state of frame t0 - 1 (0 / 1), which the range keeps
 *           until its first decisive frame (throughout, if it has none)
 * The concatenation of range calls over a partition of [0, T) is dzn_detect's output bit for bit; dzn_detect is the range
 * [0, T).  DZN_E_INVALID for t0 < 0, t1 < t0, or d_entry == NULL with t0 > 0 (d_entry is ignored when
 * t0 == 0); t1 == t0 returns DZN_OK without a launch.  Other arguments as for dzn_detect.
 */
int dzn_detect_range(const uint8_t* d_seg, int32_t C, int32_t L, int32_t S, const int32_t* d_start_frame,
                     const double* d_weight, int32_t t0, int32_t t1, int32_t tasks, float onset, float offset,
                     const uint8_t* d_entry, float* d_scores, uint8_t* d_active, void* hip_stream);

/*
 * The range form of the count -> reconstruct -> top-count chain (dzn_speaker_count + dzn_cluster_activations + the selection
 * of to_diarization), for a recording that is still arriving (diarizen_amd/live.py, LiveDiarization): frames [t0, t1) only, in
 * one call, into rows t - t0.  Per frame t, over the windows d_start_frame[0..C) that cover it:
 *   count[t]    = min(uint8(rint(sum_c sum_s seg / #covering windows)), max_count), 0 where no window covers t
 *                 SpeakerDiarizationMixin.speaker_count, PA/pipelines/utils/diarization.py:121-157 (float32 division as
 *                 dzn_speaker_count) and the cap of diarizen/pipelines/inference.py:163
 *   act[t,k]    = sum_c max_s{seg[c,t-start_c,s] : hard[c,s]==k}, integer and exact; hard < 0 or >= K is skipped
 *                 SpeakerDiarization.reconstruct, PA/pipelines/speaker_diarization.py:400-425; diarization.py:213-220
 *   active[t,k] = 1 for the min(count[t], K) largest act[t,.]     `binary[t, speakers[:c]] = 1`, diarization.py:228-236 —
 *                 zero activations are selected too when count asks for them.  Equal activations are taken in ascending k
 *                 (np.argsort(-act, kind="stable")): a fixed rule in place of numpy's build-dependent order for ties.
 * A frame's three results depend on t and on the windows covering it only, so they are final once every such window is
 * among the C — every t < the start frame of window C — and the concatenation of range calls over a partition of [0, T) is
 * the [0, T) call byte for byte.  d_seg u8 [C,L,S] (S <= 8), d_hard int8 [C,S], d_start_frame int32 [C] non-decreasing (as
 * for dzn_detect_range), 1 <= K <= 32, max_count >= 0.  d_count u8 [t1-t0], d_active u8 [t1-t0,K], d_act int32 [t1-t0,K]
 * (may be NULL).  One lane per (t, k) walks its covering windows; no atomics, no sort.  DZN_E_INVALID for t0 < 0, t1 < t0,
 * K < 1, K > 32, S > 8, max_count < 0 or NULL d_count / d_active; t1 == t0 returns DZN_OK without a launch.
 */
int dzn_diarize_range(const uint8_t* d_seg, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                      const int32_t* d_start_frame, int32_t t0, int32_t t1, int32_t K, int32_t max_count,
                      uint8_t* d_count, uint8_t* d_active, int32_t* d_act, void* hip_stream);

/*
 * dzn_diarize_range with the per-speaker activity scores of the same frames, still ONE launch (diarizen_amd/live.py,
 * LiveDiarization(scores=True)).  d_count / d_active / d_act are byte for byte what dzn_diarize_range writes for the same
 * arguments.  d_scores f32 [t1-t0, K]: row t - t0, column k holds the value dzn_speaker_scores (below) gives for frame t and
 * column k of a K-column call over the same C windows — the float32 max over the local speakers s with hard[c,s] == k of
 * d_soft[c, t-start_c, s] (NaN or no such speaker: a missing entry), accumulated over the covering windows in ascending c as
 * ((score * mask) * hamming[l]) * warm_up[l] with the two float64 [L] tables kept apart, divided as acc / max(cnt, 1e-12) in
 * float32, 0 where no valid entry landed (a column no window holds is all zeros).  d_soft f32 [C,L,S].  Lane (t, k) of
 * dzn_diarize_range's layout does the score walk inside its own loop over the covering windows: no atomics, no second pass.
 * As final as the other three outputs: a range call is the same bits as the same rows of the whole.  DZN_E_INVALID for
 * whatever dzn_diarize_range refuses and for a NULL d_soft, d_hamming, d_warm_up or d_scores; t1 == t0 returns DZN_OK
 * without a launch.  Enqueue only.
 */
int dzn_diarize_range_scores(const uint8_t* d_seg, const int8_t* d_hard, const float* d_soft, int32_t C, int32_t L, int32_t S,
                             const int32_t* d_start_frame, const double* d_hamming, const double* d_warm_up, int32_t t0,
                             int32_t t1, int32_t K, int32_t max_count, uint8_t* d_count, uint8_t* d_active, int32_t* d_act,
                             float* d_scores, void* hip_stream);

/*
 * Per-speaker activity scores (stateless, no handle): the soft scores of every window, mapped to the global clusters and
 * overlap-added.
 *   clustered[c, :, k] = max_{s : hard[c,s] == k} soft[c, :, s], NaN when window c has no local speaker in cluster k
 *                        (hard < 0 is skipped)      SpeakerDiarization.reconstruct, PA/pipelines/speaker_diarization.py:400-423
 *   scores <- Inference.aggregate(clustered, frames, hamming=True, missing=0.0, skip_average=False, warm_up=warm_up)
 *                                                   PA/core/inference.py:544-666
 * with the reference's arithmetic: per window, in window order, acc[t,k] = f32(f64(acc[t,k]) + ((score * mask) *
 * hamming[l]) * warm_up[l]) and cnt[t,k] likewise with the mask alone (a NaN entry adds nothing to either), then
 * acc / max(cnt, 1e-12) in float32, 0.0 where no non-NaN entry ever landed.
 * d_soft f32 [C,L,S] (S <= 8), d_hard int8 [C,S], d_start_frame int32 [C] non-decreasing (closest_frame, host float64, as for
 * dzn_detect), d_hamming / d_warm_up f64 [L]: two tables, multiplied in the reference's order (a pre-multiplied table does
 * not give the same bits for non-binary scores), T = output frames (frames >= T are not computed), 1 <= K <= 32,
 * d_scores f32 [T,K].  One thread per (t, k) walks its covering windows in ascending order; no atomics.
 */
int dzn_speaker_scores(const float* d_soft, const int8_t* d_hard, int32_t C, int32_t L, int32_t S,
                       const int32_t* d_start_frame, const double* d_hamming, const double* d_warm_up,
                       int32_t T, int32_t K, float* d_scores, void* hip_stream);

/*
 * The matching step of the Resegmentation pipeline (stateless, no handle; csrc/reseg.hip): per window, the disagreement
 * counts between the speakers of a given diarization and the model's local speakers — the cost matrices of the reference's
 * per-window loop, as exact integers.
 *   n = max(K, S): the narrower side is widened with zero columns      PA/pipelines/resegmentation.py:217-228
 *   count[c, i, j] = #{ l < Lt : refpad[d_row[c] + l, i] != segpad[c, l0 + l, j] }
 *                    <- the loop over windows, resegmentation.py:230-243; permutate's cost matrix, PA/utils/permutation.py:
 *                       131-157, with mae_cost_func = torch.mean(|Y - y|) (permutation.py:83-95): the caller's
 *                       float32(count) / float32(Lt) is that mean on {0,1} data
 *   frames [l0, l0 + Lt) of every window are those Inference.trim keeps      PA/core/inference.py:669-713
 * d_seg u8 [C,L,S] hard decisions; d_ref u8 [Tr,K] the given diarization on the frame grid (may be NULL when K == 0 or
 * Tr == 0), rows at or beyond Tr read as inactive; d_row int32 [C] the first reference row of every window (the loose crop of
 * resegmentation.py:234, computed by the caller in float64); d_count int32 [C,n,n].  One workgroup per window, no atomics.
 * Enqueue-only.  DZN_E_INVALID, nothing launched: n > 32, S < 1, Lt < 1, l0 < 0, l0 + Lt > L, C < 0, K < 0, Tr < 0 or a null
 * pointer; C == 0 returns DZN_OK without a launch.  The assignment (scipy.optimize.linear_sum_assignment) is the caller's.
 */
int dzn_match_counts(const uint8_t* d_seg, const uint8_t* d_ref, int32_t C, int32_t L, int32_t S, int32_t Tr, int32_t K,
                     const int32_t* d_row, int32_t l0, int32_t Lt, int32_t* d_count /* [C, n, n] */, void* hip_stream);

/* Copy a named intermediate activation of the LAST forward to host (debug / parity
 * tests).  *n_elems receives the element count; host_out may be NULL to query. */
int dzn_debug_fetch(dzn_handle* h, const char* name, float* host_out, int64_t cap,
                    int64_t* n_elems);

/* dzn_embed_forward skips the ResNet trunk for windows in which no speaker is active (their embeddings are seg_1's
 * bias: zero weights pool to zero, PA/models/blocks/pooling.py:44-131).  The subset is chosen ON THE DEVICE (r4): the
 * forward reads nothing back and stays enqueue-only.  Counters since dzn_create: windows seen by dzn_embed_forward /
 * windows whose trunk pass was skipped; they live on the device, so THIS call synchronises the device (diagnostics;
 * no reference counterpart).  DZN_EMB_NO_SKIP in the environment at dzn_create switches the subset off. */
int dzn_embed_skip_stats(const dzn_handle* h, int64_t* windows, int64_t* skipped);

int dzn_num_ignored(const dzn_handle* h);
int64_t dzn_workspace_bytes(const dzn_handle* h);
const char* dzn_last_error(const dzn_handle* h); /* h may be NULL: last create error */
int dzn_destroy(dzn_handle* h);
const char* dzn_version(void);

/*
 * Host-clustering accelerator.  Drop-in for
 *     scipy.cluster.hierarchy.linkage(emb, method="centroid", metric="euclidean")
 * as called by AgglomerativeClustering.cluster (PA/pipelines/clustering.py:407-416) and by the AHC
 * initialisation of VBxClustering (PA/pipelines/clustering.py:656-658): h_emb is a HOST float32
 * [n, dim] matrix (rows already unit-normalised by the caller, as in the reference), h_Z receives the
 * scipy dendrogram [n-1, 4] float64 (ids, ids, distance, size).  The n x n float64 distance matrix
 * lives in HBM (8 n^2 bytes -> DZN_E_NOMEM when it does not fit).  Blocking; device < 0 = current.
 */
int dzn_linkage_centroid(const float* h_emb, int32_t n, int32_t dim, double* h_Z, int32_t device);

/* Row f1, assignment step: scipy.spatial.distance.cdist(emb, centroids, metric="cosine") of
 * BaseClustering.assign_embeddings (pyannote/audio/pipelines/clustering.py:207-216) on the device: float64, row
 * norms, then 1 - clip(dot / (|u||v|)) with in-order sums and no FMA (agrees with scipy to 2e-15 on distances of
 * order 1; identical rows give identical scores).  HOST pointers: h_emb f32 [n, dim], h_cent f64 [k, dim],
 * h_dist f64 [n, k].  Blocking; device < 0 = current.  Rows with a NaN / zero norm give NaN like scipy. */
int dzn_cdist_cosine(const float* h_emb, int32_t n, int32_t dim, const double* h_cent, int32_t k, double* h_dist,
                     int32_t device);

/* (r5) dzn_linkage_centroid / dzn_cdist_cosine work on their OWN non-blocking, highest-priority stream and carve their
 * buffers from one grow-only arena per device (they are called from the pipeline's host stage, which may run in a second
 * thread while the engine executes the next recording's device stage: no null-stream ordering behind the engine's queue, no
 * hipFree).  The arena is re-allocated only when a call needs more than any call before it; these return it / report it.
 * A dzn_vbx_* state is carved from a second arena of the same context (leased to one state at a time — a second live state gets a
 * block of its own — and kept while a state holds it) and works on the same stream.
 * device < 0 in dzn_host_workspace_release = every device.  No reference counterpart (scipy owns its host buffers). */
int dzn_host_workspace_release(int32_t device);
int64_t dzn_host_workspace_bytes(int32_t device);

/* Row f1, VBx: the variational-Bayes mixture of diarizen/clustering/VBx.py:27-125 (loopProb = 0 branch :99-107, the
 * one VBxClustering.__call__ runs) with its two E-sized passes per iteration on the device (csrc/vbx.hip), float64.
 * The K x D statistics pass through the host, which keeps the reference's expressions for invL / alpha / ELBO and its
 * stopping rule (diarizen_amd/clustering.py:vb_gmm).  HOST pointers, blocking calls; device < 0 = current.
 *   dzn_vbx_create   X f64 [E, D] (PLDA-space features), Phi f64 [D], gamma0 f64 [E, K] -> opaque state
 *   dzn_vbx_stats    h_stats f64 [K, D + 1] <- (gamma^T rho | column sums of gamma), rho = X sqrt(Phi)
 *   dzn_vbx_estep    alpha f64 [K, D], ck f64 [K] = 0.5 sum_d (invL + alpha^2) Phi, lpi f64 [K] = log(pi + 1e-8):
 *                    gamma <- softmax_k(Fa (rho alpha^T - ck + G) + lpi); *h_total = sum_e logsumexp_k(...)
 *   dzn_vbx_gamma    h_gamma f64 [E, K] <- the current responsibilities
 */
int dzn_vbx_create(const double* h_X, const double* h_Phi, const double* h_gamma0, int32_t E, int32_t D, int32_t K,
                   int32_t device, void** out_state);
int dzn_vbx_stats(void* state, double* h_stats);
int dzn_vbx_estep(void* state, const double* h_alpha, const double* h_ck, const double* h_lpi, double Fa,
                  double* h_total);
int dzn_vbx_gamma(void* state, double* h_gamma);
int dzn_vbx_destroy(void* state);

/* Speaker identification (csrc/gallery.hip): a device-resident gallery of enrolled voiceprints and one cosine
 * search over it.  No reference counterpart: the reference ends at anonymous cluster labels.  A voiceprint is a cluster
 * centroid of the embeddings the engine already produces, so enrolment and test live in the same space.
 *   storage  fp32 [capacity, dim] (dim a multiple of 16, 16 .. 512), every row L2-normalised at put: norm in float64 (in-order
 *            sum, as dzn_cdist_cosine's row norms), quotient rounded once to fp32; one validity byte per slot.  The gallery's
 *            own allocation, made at create and freed at destroy; dzn_host_workspace_release leaves it alone.
 *   search   queries normalised the same way; score = fp32 dot product on the f32-input MFMA (one fmaf chain of dim products,
 *            |score - float64 cosine| <= (dim + 8) 2^-24).  Per query the top_n VALID rows by (score descending, slot
 *            ascending): duplicated rows tie, the lower slot first; entries beyond the number of valid rows are slot -1,
 *            score -inf.  h_dense (optional) receives every score, [Q, rows] with rows = highest slot ever put + 1
 *            (dzn_gallery_rows): the same bits the selection saw, -inf at dropped or never-put slots.
 * HOST pointers, blocking calls on the host stage's stream and arena (as dzn_cdist_cosine: callable from a second thread beside
 * the engine).  DZN_E_INVALID, nothing written: null pointers, Q < 1, top_n < 1 or > max_top_n (32), a slot range outside the
 * capacity, a put row or a query that is all zero or not finite (checked on the host before any upload).
 *   dzn_gallery_geometry        tile_rows: rows per workgroup tile; sweep_rows: rows one pass of the launched grid covers on this
 *                               device; query_group: queries that share one sweep (Q beyond it loops); max_top_n
 *   dzn_gallery_last_launch_ms  HIP-event time of the last search's launches (scans + merges, without the copies);
 *                               merge_ms (optional): the share of the last group's merge */
int dzn_gallery_create(int32_t device, int32_t dim, int64_t capacity, void** out);
int dzn_gallery_put(void* g, int64_t slot, const float* h_vecs, int64_t count);
int dzn_gallery_drop(void* g, int64_t slot, int64_t count);
int dzn_gallery_search(void* g, const float* h_queries, int32_t Q, int32_t top_n, float* h_scores, int64_t* h_slots,
                       float* h_dense);
int dzn_gallery_geometry(const void* g, int32_t* tile_rows, int32_t* sweep_rows, int32_t* query_group, int32_t* max_top_n);
int dzn_gallery_rows(const void* g, int64_t* rows);
int dzn_gallery_last_launch_ms(const void* g, float* ms, float* merge_ms);
int dzn_gallery_destroy(void* g);

/* Linking speakers across recordings (csrc/linkage.hip): complete-linkage agglomerative clustering of the
 * voiceprints of a whole corpus under a cannot-link constraint, cut at a distance threshold.  No reference counterpart: the
 * reference's labels restart at 0 in every recording.  The entry does what scipy does with
 *     y = pdist(E.astype(float64), "cosine");  y[pairs with h_group[i] == h_group[j]] = 4.0;  Z = linkage(y, "complete")
 * stopped early: the first *h_merges rows of h_Z are exactly the merges of height <= threshold, in scipy's order and with
 * scipy's ids and sizes (no exact ties among the allowed distances assumed); rows past *h_merges are unspecified.
 *   distances  float64 from the float32 rows: row norms as dzn_cdist_cosine, 1 - clip(dot / (|u||v|)), in-order sums;
 *              |d - true| <= 2 (dim + 8) 2^-53.  Two rows of one group are set to 4.0: finite, above every cosine distance
 *              (<= 2), so the pair can never merge at a threshold in (0, 2] — and with complete linkage neither can any two
 *              clusters that hold such a pair.
 *   loop       the step loop of dzn_linkage_centroid with the update v = max(d_xi, d_yi); it ends at the first closest pair
 *              above the threshold.  The n x n float64 matrix lives in the host stage's arena (8 n^2 bytes -> DZN_E_NOMEM when
 *              it does not fit); same stream, mutex and blocking behaviour as dzn_linkage_centroid.
 * HOST pointers: h_emb f32 [n, dim], h_group i32 [n] (any integers; equal = same recording), h_Z f64 [n - 1, 4].
 * DZN_E_INVALID, nothing written: null pointers, n < 2, dim < 1, threshold not in (0, 2], a row that is all zero or not finite
 * (checked on the host before any upload).
 *   dzn_link_speakers_last  diagnostics of the last call of the process (any pointer may be NULL): step launches queued
 *                           (surplus ones included), merges, row rescans, HIP-event time of the distance kernel alone */
int dzn_link_speakers(const float* h_emb, const int32_t* h_group, int32_t n, int32_t dim, double threshold, double* h_Z,
                      int32_t* h_merges, int32_t device);
int dzn_link_speakers_last(int64_t* launches, int32_t* merges, int32_t* rescans, float* pdist_ms);

/* A speaker registry (csrc/registry.hip): the incremental counterpart of dzn_link_speakers.  The voiceprints
 * linked so far stay on the device, every stored row under an identity number that the caller chose; the Q voiceprints of a new
 * recording are matched against all of them in one sweep:
 *     D[k][i] = max over the stored rows r with identity i of cosdist(q_k, E_r)
 * — the complete-linkage distance of query k to identity i — and of that table the entries <= threshold come back as
 * (k, i, d) triples.  The assignment rule that continues complete linkage from them is the caller's (diarizen_amd/registry.py).
 *   storage    fp32 [capacity, dim] as given (dim a multiple of 4, 4 .. 1024) and the float64 row norms: the registry's own
 *              allocation, made at create and freed at destroy; dzn_host_workspace_release leaves it alone.  Identity numbers
 *              are any int32 in [0, 2^31 - 2]; numbers without a stored row are allowed (I = the highest number + 1).
 *   distances  float64 from the float32 rows, exactly dzn_cdist_cosine's expression: row norms with in-order sums,
 *              1 - clip(dot / (|q||e|)), one in-order sum over dim per (query, row); |d - true| <= 2 (dim + 8) 2^-53.  The result
 *              does not depend on the launch geometry, on Q or on the order of earlier calls (max is order-free; no float atomics).
 *   append     count rows with their identity numbers.  DZN_E_NOMEM when they do not fit the capacity, DZN_E_INVALID for a
 *              negative number or a row that is all zero or not finite; a refused call stores nothing.  count = 0 is a no-op.
 *   match      h_queries f32 [Q, dim] -> *h_count = the number of entries <= threshold, and the first min(*h_count, max_out) of
 *              them in h_k / h_i (int32) / h_d (float64), sorted by (k, i).  *h_count > max_out: call again with room for all
 *              (which of them were returned is unspecified then).  h_dense (optional) receives the whole table, float64 [Q, I],
 *              +inf in the column of a number that holds no row.  Q = 0 or an empty registry: *h_count = 0, nothing launched.
 *              DZN_E_INVALID, nothing written: null pointers, Q < 0, max_out < 0, threshold not in (0, 2], a query that is all
 *              zero or not finite.
 * HOST pointers, blocking calls on the host stage's stream and arena (as dzn_cdist_cosine: callable from a second thread beside
 * the engine).
 * One append / match / rows / last_launch_ms of a handle runs at a time (they may be called from several threads); destroy waits
 * for a call in flight, and no call on the handle may begin once destroy has.  capacity: at most 2 114 445 312 rows (the
 * segment ids of the member index are int32).
 *   dzn_registry_rows            stored rows; identities (optional): I
 *   dzn_registry_last_launch_ms  HIP-event time of the last match's launches (sweeps + reduce, without copies and index upload) */
int dzn_registry_create(int32_t device, int32_t dim, int64_t capacity, void** out);
int dzn_registry_append(void* r, const float* h_vecs, int64_t count, const int32_t* h_identity);
int dzn_registry_match(void* r, const float* h_queries, int32_t Q, double threshold, int32_t max_out, int32_t* h_k, int32_t* h_i,
                       double* h_d, int32_t* h_count, double* h_dense);
int dzn_registry_rows(const void* r, int64_t* rows, int64_t* identities);
int dzn_registry_last_launch_ms(const void* r, float* ms);
int dzn_registry_destroy(void* r);

/* Row f3, audio ingest: native FLAC decoder (csrc/flac.cpp, host code; the reference reads whatever torchaudio.load does,
 * diarizen/pipelines/inference.py:127 — WAV is parsed in diarizen_amd/audio.py, FLAC here).  Frame-header CRC-8 and frame
 * CRC-16 are verified while decoding; the caller checks the STREAMINFO MD5 (audio.load_flac does).
 *   dzn_flac_info    stream parameters from STREAMINFO (any output pointer may be NULL); total_samples 0 = unknown
 *   dzn_flac_decode  out = int32 [capacity_samples][channels], interleaved, sign-extended; *decoded = samples per channel.
 * Returns DZN_OK, DZN_E_INVALID (not FLAC / corrupt / unsupported), DZN_E_NOMEM (capacity too small). */
int dzn_flac_info(const uint8_t* data, size_t n, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample,
                  int64_t* total_samples, uint8_t* md5_16);
int dzn_flac_decode(const uint8_t* data, size_t n, int32_t* out, int64_t capacity_samples, int64_t* decoded);

/* Row f3, audio ingest: the polyphase sinc resampler on the device (csrc/resample.hip; stateless, no handle), i.e.
 * torchaudio.functional.resample as Audio.downmix_and_resample applies it, PA/core/io.py:214-218 (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99; the host form is diarizen_amd/audio.py:resample).  With o = orig / gcd, n = new / gcd,
 * K = 2 width + o, output sample m = f n + p of a recording of total_len = T input samples is
 *     y[m] = sum_{j < K} bank[p][j] * x[f o + j - width],      x = 0 outside [0, T),      0 <= m < ceil(n T / o)
 * in float32: one accumulator, acc = fmaf(bank[p][j], x[..], acc) for j = 0 .. K-1.  That order depends on m alone, so a call
 * for a range of a recording returns the bits of the same slice of a call for all of it.  One launch, enqueue-only, on
 * `hip_stream` of `device` (< 0 = current) writes d_dst f32 [m1 - m0] = y[m0 .. m1).
 *   d_src            device frames src_first_index .. src_first_index + src_len of the recording, as the file stores them
 *                    (src_len counts frames: src_len * channels samples); the staging loop decodes what it reads, every
 *                    conversion is exact in float32 except the int32 one, which rounds to nearest even as numpy's astype:
 *                      DZN_SRC_F32   0  float32 mono (channels = 1)            as is
 *                      DZN_SRC_S16   1  int16, interleaved over `channels`     v * 2^-15 (audio.load_wav of a PCM16 file)
 *                      DZN_SRC_U8    2  uint8 offset-binary, interleaved       (v - 128) * 2^-7
 *                      DZN_SRC_S24   3  24-bit packed little-endian            sign-extended v * 2^-23
 *                      DZN_SRC_S32   4  int32, interleaved                     (float)v * 2^-31
 *                      DZN_SRC_F32I  5  float32, interleaved over `channels`   as is
 *                      DZN_SRC_ULAW  6  G.711 mu-law byte, interleaved         audio.ulaw_table()[v] * 2^-15
 *                      DZN_SRC_ALAW  7  G.711 A-law byte, interleaved          audio.alaw_table()[v] * 2^-15
 *   channel          0 .. channels - 1: that channel of every frame; DZN_CHANNEL_DOWNMIX (-1): audio.downmix of the frame,
 *                    i.e. a float32 running sum over the decoded channels 0, 1, .. then ONE IEEE float32 division by
 *                    (float)channels (the channel itself when channels = 1)
 *   d_bank           device f32 [K][n], TAP-major: d_bank[j * n + p] = bank[p][j] (audio.resample_bank, transposed)
 * The taps walk the decoded samples in the same order for every format, so a stored-format call returns the bits of the
 * float32 call on the host-decoded channel.
 * Returns DZN_E_INVALID with a dzn_last_error(NULL) message, and launches nothing, when src_format is none of the above or is
 * DZN_SRC_F32 with channels != 1, when channel < -1 or channel >= channels, when the span given does not cover what [m0, m1)
 * reads inside [0, T), when m1 > ceil(n T / o), or when o / n is so large that the input of one tile does not fit in 64 KiB
 * of LDS.  dzn_resample_tile: output samples per workgroup (tests place ranges on it). */
#define DZN_SRC_F32 0
#define DZN_SRC_S16 1
#define DZN_SRC_U8 2
#define DZN_SRC_S24 3
#define DZN_SRC_S32 4
#define DZN_SRC_F32I 5
#define DZN_SRC_ULAW 6
#define DZN_SRC_ALAW 7
#define DZN_SRC_FORMATS 8          /* codes 0 .. 7 */
#define DZN_CHANNEL_DOWNMIX (-1)
int dzn_resample(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int32_t channel,
                 int64_t src_first_index, int64_t src_len, int64_t total_len, const float* d_bank, int32_t o, int32_t n,
                 int32_t width, int64_t m0, int64_t m1, float* d_dst, void* hip_stream);
int32_t dzn_resample_tile(void);

/* The decode half of dzn_resample on its own, for frames that are already at the model's rate (the bank for equal rates is a
 * low-pass, not the identity): d_dst f32 [frames] = the channel choice of the `frames` stored frames at d_src, with the
 * DZN_SRC_* codes, DZN_CHANNEL_DOWNMIX and the conversions above (every one exact but int32, which rounds to nearest even;
 * the downmix is the float32 running sum over channels 0, 1, .. then ONE IEEE division by (float)channels), i.e. the bits of
 * the host decode (audio._decode_frames, then select_channel or downmix); DZN_SRC_F32 is a plain copy.  One launch (one
 * stored frame per lane), enqueue-only, on `hip_stream` of `device` (< 0 = current); frames = 0 is DZN_OK and launches
 * nothing.  Returns DZN_E_INVALID with a dzn_last_error(NULL) message, and launches nothing, for what dzn_resample refuses
 * (src_format, DZN_SRC_F32 with channels != 1, channel) and for a d_src that is not aligned to the sample size (2 bytes for
 * int16, 4 for int32 / float32; 8-bit, 24-bit and G.711 samples take any address). */
int dzn_decode(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int32_t channel, int64_t frames,
               float* d_dst, void* hip_stream);

/* Array recordings (csrc/beamform.hip; diarizen_amd/audio.py: Beamform, BeamformedSource): GCC-PHAT
 * delay-and-sum over C = `channels` microphones, 2 <= C <= 64, into the one channel the engine diarizes.  Both calls are
 * stateless.  Input is PLANAR float32: d_x[c * ch_stride + (i - x_first)] is sample i of channel c for
 * x_first <= i < x_first + x_len of a recording of T samples (x = 0 outside [0, T)); ch_stride >= x_len.
 * With hop H a power of two in [256, 4096], W = 2 H, the recording has nb = ceil(T / H) + 1 blocks; frame b is samples
 * (b - 1) H .. (b + 1) H - 1 times the periodic Hann window 0.5 - 0.5 cos(2 pi i / W).
 *
 * dzn_beamform_delays: for the blocks [b0, b1) and every channel c != ref, X = FFT_W(frame), P = X_c conj(X_ref),
 * G = P / |P| (0 where P is 0), g[l] = (1 / W) sum_k G_k e^{+2 pi i k l / W} (circular), and
 *     d_lag  i32 [channels][b1 - b0]   the l in [-max_lag, max_lag] with the largest g[l]; ties go to the first of
 *                                      0, -1, +1, -2, +2, ..; with x_c[i] = s[i - d] the peak sits at l = +d
 *     d_peak f32 [channels][b1 - b0]   g[lag]
 * The row of `ref` is 0 / 0, and so is every block whose frames are all zero.  1 <= max_lag <= H / 2.
 * d_twiddle f32 [W / 2][2] = (cos, -sin)(2 pi k / W), computed in float64 and rounded once (audio.beamform_twiddle).
 * One launch, enqueue-only, on `hip_stream` of `device` (< 0 = current).
 *
 * dzn_beamform_sum: d_dst f32 [n1 - n0] = y[n0 .. n1) with, for n in [b H, (b + 1) H),
 *     S_b(n) = (sum_{c = 0 .. C-1} x_c[n + delay[c][b]]) / C      float32 running sum in ascending c, ONE IEEE division
 *     y[n]   = a + w (v - a),  a = S_b(n), v = S_{b+1}(n), w = (n - b H) / H      three separately rounded float32 operations
 * d_delay i32 [channels][num_blocks] holds the smoothed delays of the WHOLE recording (num_blocks = nb; audio.smooth_delays),
 * |delay| <= H / 2.  The delays decide which samples are read, so the call copies the columns its range uses back to the host
 * (a few KB) and checks them before it launches: it waits for what `hip_stream` holds up to d_delay; the launch itself is
 * enqueued.  dzn_beamform_tile: output samples per workgroup (tests place ranges on it).
 *
 * Results depend on the inputs and parameters alone, not on the range asked for: a range call returns the bits of the same
 * slice of a whole-recording call.  Both return DZN_E_INVALID with a dzn_last_error(NULL) message, and launch nothing, for
 * channels outside [2, 64], ref outside the channels, a hop that is not a power of two in [256, 4096], max_lag outside
 * [1, H / 2], blocks outside [0, nb] or samples outside [0, T], num_blocks != nb, a delay beyond H / 2 in the columns used, and
 * an x span that does not cover what the range reads inside [0, T): samples (b0 - 1) H .. b1 H - 1 for the delays, n + delay
 * of either block for the sum. */
int dzn_beamform_delays(int32_t device, const float* d_x, int32_t channels, int64_t ch_stride, int64_t x_first, int64_t x_len,
                        int64_t T, int32_t ref, int32_t hop, int32_t max_lag, const float* d_twiddle, int64_t b0, int64_t b1,
                        int32_t* d_lag, float* d_peak, void* hip_stream);
int dzn_beamform_sum(int32_t device, const float* d_x, int32_t channels, int64_t ch_stride, int64_t x_first, int64_t x_len,
                     int64_t T, int32_t hop, const int32_t* d_delay, int64_t num_blocks, int64_t n0, int64_t n1, float* d_dst,
                     void* hip_stream);
int32_t dzn_beamform_tile(void);

/* Array FEEDS (csrc/beamform_live.hip; audio.Beamform(causal=True), audio.causal_delays, audio.ArrayFeedPlanner,
 * streaming.WaveIngest): the same blocks, frames, raw lag / peak and alignment pass as above, with a delay rule
 * that looks at no later block and is tracked on the device, so that a live session beamforms in stream order.
 *
 * Causal delays.  For a channel c != ref and blocks b = 0, 1, ..:
 *     reliable[b] = frame b holds at least H samples of the recording (min(T, (b + 1) H) - max(0, (b - 1) H) >= H)
 *                   and peak[c][b] >= min_peak (float32)
 *     held[b]     = lag[c][b] if reliable[b], else held[b - 1]; held[-1] = 0 (no backward fill: a channel aligns from its
 *                   first reliable block on)
 *     delay[c][b] = the median of held[b - 4 .. b], where held[k] = held[0] for k < 0 (a TRAILING median of 5 whose left
 *                   edge repeats the first entry)
 * and the row of `ref` is 0.  delay[c][b] depends on blocks <= b alone and |delay| <= max_lag.  A change of delay takes effect
 * two blocks late (the trailing median needs three of five entries): 0.5 s at the default hop.
 *
 * Schedule.  After R frames of a feed block b is complete when R >= (b + 1) H: nc = floor(R / H) blocks are.  A complete
 * frame holds the same samples whatever the eventual length T, so its lag, peak and reliability are those of the
 * whole-recording computation.  Output sample n of block b reads n + delay of blocks b and b + 1, below (b + 2) H, so the
 * samples below beam_ready(R) = max(0, nc - 1) H are final: output lags the feed by less than 2 H frames.  At the end of the
 * stream the blocks nc .. ceil(T / H) are evaluated with the true T (ragged frames, zero outside [0, T)) and the samples
 * [beam_ready, T) made.
 *
 * dzn_decode_planar: d_dst f32 [channels][ch_stride], d_dst[c * ch_stride + r] = sample c of stored frame r for r < frames
 * (ch_stride >= frames; the floats behind `frames` in a row are not touched), with the DZN_SRC_* codes and conversions of
 * dzn_decode bit for bit, in ONE pass over the source (one frame per lane).  One launch, enqueue-only; frames = 0 is DZN_OK and
 * launches nothing.  It refuses what dzn_decode refuses (src_format, DZN_SRC_F32 with channels != 1, a misaligned d_src) and
 * ch_stride < frames.
 *
 * dzn_beamform_track: the causal rule over blocks [b0, b1).  d_lag i32 / d_peak f32 are compact arrays of row stride nblk
 * whose column 0 is block b0 (what dzn_beamform_delays writes for blocks [b0, b1): nblk = b1 - b0; nblk > b1 - b0 reads the
 * leading columns of wider rows).  d_state i32 [channels][DZN_BEAMFORM_STATE_INTS] is the tracker's state — per channel the
 * held values of the four blocks before b0, oldest first, then the number of blocks seen — ZEROED by the caller before block
 * 0 and otherwise only passed on.  d_delay i32 [channels][delay_stride]: columns b0 .. b1 - 1 are written.  The kernel is a
 * function of (state, columns) alone: tracking [0, nb) at once or in any partition into consecutive calls gives the same table
 * and the same final state.  Lags and state are clamped to [-H / 2, H / 2] as they are read.  *h_seen is the HOST's count of
 * blocks tracked on this state (0 for a zeroed state): b0 must equal it — DZN_E_INVALID otherwise — and the call sets it to
 * b1; device memory is never read back.  One launch of one wavefront (a lane per channel, sequential over the blocks),
 * enqueue-only, plain loads and stores.  Refused: channels outside [2, 64], ref outside the channels, a bad hop, T < 0,
 * b0 < 0, b1 < b0, b1 - b0 > nblk, b1 > delay_stride, b1 > ceil(T / H) + 1, b0 != *h_seen, null pointers.
 *
 * dzn_beamform_feed: what ONE live call enqueues on `hip_stream`, in order: dzn_decode_planar of the uploaded frames
 * src_first .. src_first + src_frames into d_planar [channels][ch_stride]; GCC-PHAT (the kernel of dzn_beamform_delays) of
 * blocks [b0, b1) into d_lag / d_peak [channels][b1 - b0] (temporaries of blk_cap blocks per channel); the tracker (lags
 * clamped to max_lag) into columns [b0, b1) of d_delay i32 [channels][table_blocks]; the alignment pass (the kernel of
 * dzn_beamform_sum) for samples [n0, n1) into d_dst f32 [n1 - n0], reading the device-resident table with num_blocks =
 * table_blocks.  T is the number of frames received when the call is made (the true length at the end of the stream).  No
 * synchronisation, no allocation, no read-back: every buffer is the caller's, and the call validates from its arguments alone
 * — the tracker bounds the delays by max_lag, so the span the sum can read is [n0 - max_lag, n1 + max_lag) inside [0, T).
 * Refused, with a dzn_last_error(NULL) message and nothing enqueued: what dzn_decode_planar, dzn_beamform_delays and
 * dzn_beamform_track refuse; b1 - b0 > blk_cap or b1 > table_blocks; samples outside [0, T] or that use a block that is not
 * tracked after this call ((n1 - 1) / H + 1 >= b1); an uploaded span that does not cover samples (b0 - 1) H .. b1 H - 1 of
 * the blocks or [n0 - max_lag, n1 + max_lag) of the samples, inside [0, T).
 * Measured on one MI355X (scripts/beamform_live_timing.py): the upload and this call for a 10 s slot of int16
 * frames take 0.13 / 0.46 / 3.6 ms of device time for 2 / 8 / 64 channels at 16 kHz and 0.19 / 0.61 / 4.8 ms at 48 kHz
 * (with the resampler), against 0.04 - 1.1 ms for one channel of the same frames.  No speed is promised or tested. */
#define DZN_BEAMFORM_STATE_INTS 5
int dzn_decode_planar(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int64_t frames, float* d_dst,
                      int64_t ch_stride, void* hip_stream);
int dzn_beamform_track(int32_t device, const int32_t* d_lag, const float* d_peak, int64_t nblk, int32_t channels, int32_t ref,
                       int32_t hop, int64_t T, float min_peak, int64_t b0, int64_t b1, int32_t* d_state, int64_t* h_seen,
                       int32_t* d_delay, int64_t delay_stride, void* hip_stream);
int dzn_beamform_feed(int32_t device, const void* d_src, int32_t src_format, int32_t channels, int64_t src_first,
                      int64_t src_frames, int64_t T, int32_t ref, int32_t hop, int32_t max_lag, float min_peak,
                      const float* d_twiddle, float* d_planar, int64_t ch_stride, int32_t* d_lag, float* d_peak, int64_t blk_cap,
                      int64_t b0, int64_t b1, int32_t* d_state, int64_t* h_seen, int32_t* d_delay, int64_t table_blocks,
                      int64_t n0, int64_t n1, float* d_dst, void* hip_stream);

/* Live hub (diarizen_amd/hub.py): the ingest of MANY sessions in one launch (csrc/ingest.hip).  A descriptor is what one
 * dzn_resample or dzn_decode call takes; its source lies in one staging buffer, its bank in one buffer of banks, its output in
 * one pooled buffer f32 [pool_rows][row_floats] (a row per session: the recording so far, zeros behind it).  Fixed-width
 * fields, 96 bytes, no padding:
 *   src_offset        byte offset of the stored frames inside d_stage (the address must be aligned to the sample size:
 *                     2 bytes for int16, 4 for int32 / float32; the hub pads every call to 16 bytes)
 *   src_first_index,  the frames at src_offset are frames src_first_index .. + src_len of a recording of total_len frames so
 *   src_len,          far (dzn_resample's arguments).  A decode descriptor holds the frames it decodes and nothing else:
 *   total_len         src_len = m1 - m0; src_first_index and total_len are not read
 *   m0, m1            the output samples [m0, m1) it makes; m1 = m0 is legal and owns no tile
 *   bank_offset       float offset of its bank f32 [K][n] (tap-major, as dzn_resample takes it) inside d_banks;
 *                     negative: decode only (a feed at the model's rate; o, n, width are not read)
 *   dst_offset        float offset of y[m0] inside d_pool; [dst_offset, dst_offset + m1 - m0) must lie in ONE row
 *   src_format,       DZN_SRC_* / channels >= 1 / a channel index or DZN_CHANNEL_DOWNMIX, as dzn_resample takes them
 *   channels, channel
 *   o, n, width       the ratio and filter half-width of the bank
 *   tile0             the tile prefix: the number of tiles owned by the descriptors before this one, where a descriptor owns
 *                     ceil((m1 - m0) / dzn_resample_tile()) tiles (the caller writes it, the call verifies it)
 *   reserved          0 */
typedef struct dzn_ingest_desc {
  int64_t src_offset;
  int64_t src_first_index;
  int64_t src_len;
  int64_t total_len;
  int64_t m0;
  int64_t m1;
  int64_t bank_offset;
  int64_t dst_offset;
  int32_t src_format;
  int32_t channels;
  int32_t channel;
  int32_t o;
  int32_t n;
  int32_t width;
  int32_t tile0;
  int32_t reserved;
} dzn_ingest_desc;

/* ONE launch, enqueue-only, on `hip_stream` of `device` (< 0 = current): one workgroup per tile of dzn_resample_tile() output
 * samples (a decode descriptor: frames) of one descriptor, found by a wave-uniform search over tile0.  The arithmetic is that
 * of the single calls — one fp32 accumulator over j = 0 .. K-1, the downmix a running fp32 sum and one IEEE division, zeros
 * outside [0, total_len) — so every output sample has the bits dzn_resample / dzn_decode give for the same arguments.  Dynamic
 * LDS is the largest tile image of the table.  Pool floats outside every [dst_offset, dst_offset + m1 - m0) are not touched.
 *   d_stage, stage_bytes   the staging buffer on the device and its size
 *   h_desc, d_desc         the table of num_desc descriptors: h_desc is the host's image of it (validated here, it may be the
 *                          pinned buffer the table was uploaded from), d_desc the device copy the kernel reads
 *   d_banks, bank_floats   the buffer of banks and its size in floats
 *   d_pool, pool_rows,     the pooled output
 *   row_floats
 * num_desc = 0, or a table without tiles, launches nothing and returns DZN_OK.  Anything dzn_resample / dzn_decode would
 * refuse in a descriptor — and a source that leaves the staging buffer or is not aligned to its 2- or 4-byte samples, a bank
 * that leaves d_banks, an output range that leaves its pool row, a tile0 that is not the prefix — makes the WHOLE call return
 * DZN_E_INVALID with a dzn_last_error(NULL) message that names the descriptor index, and launches nothing. */
int dzn_ingest_many(int32_t device, const void* d_stage, int64_t stage_bytes, const dzn_ingest_desc* h_desc,
                    const dzn_ingest_desc* d_desc, int32_t num_desc, const float* d_banks, int64_t bank_floats, float* d_pool,
                    int64_t pool_rows, int64_t row_floats, void* hip_stream);

/* The dense batch of windows the forward reads: d_dst f32 [B][window], d_dst[b][:] = d_pool[offsets[b] .. offsets[b] + window).
 * h_offsets is the host's image of d_offsets (int64 [B], in floats); every window must lie inside the pool_floats floats of
 * d_pool (DZN_E_INVALID with a dzn_last_error(NULL) message otherwise; nothing is launched).  Rows whose source and destination
 * are both 16-byte aligned move 16 bytes per access (live offsets are multiples of the step), the others take a scalar path.
 * One launch, enqueue-only, on `hip_stream` of `device` (< 0 = current); B = 0 launches nothing; B <= 65535. */
int dzn_gather_windows(int32_t device, const float* d_pool, int64_t pool_floats, const int64_t* h_offsets,
                       const int64_t* d_offsets, int32_t B, int32_t window, float* d_dst, void* hip_stream);

/* Live hub, array feeds (diarizen_amd/hub.py, csrc/beamform_many.hip): the beamforming of MANY array sessions
 * in one fixed set of four launches.  A descriptor is what ONE dzn_beamform_feed call takes; its stored frames lie in one
 * staging buffer, its twiddle table in one buffer of tables, its planar decode and lag / peak temporaries in scratch shared by
 * the table, its tracker state and delay table in one buffer each (a region per session), and its output in the pooled session
 * buffer or in a pool of beamformed staging buffers.  Fixed-width fields, 208 bytes, no padding:
 *   src_offset        byte offset of the stored frames inside d_stage (aligned to the sample size, as dzn_ingest_desc)
 *   src_first,        the frames at src_offset are frames src_first .. + src_frames of a feed of T frames so far (the true
 *   src_frames, T     length at the end of the stream): dzn_beamform_feed's arguments
 *   twiddle_offset    float offset of the table f32 [hop][2] of this hop inside d_twiddles (audio.beamform_twiddle)
 *   planar_offset,    the planar decode f32 [channels][ch_stride] lies at float planar_offset of d_planar; ch_stride >=
 *   ch_stride         src_frames.  Regions of different descriptors must not overlap (they are written in one launch)
 *   lag_offset,       lag i32 / peak f32 [channels][b1 - b0] lie at element lag_offset of d_lag / d_peak, in a region of
 *   blk_cap           channels * blk_cap elements (b1 - b0 <= blk_cap); regions must not overlap
 *   b0, b1            the blocks [b0, b1) the call completes
 *   seen              the HOST's count of blocks tracked on the state at state_offset: b0 must equal it.  The caller advances
 *                     its count to b1 after a successful call; device memory is never read back
 *   state_offset      int offset of the tracker state i32 [channels][DZN_BEAMFORM_STATE_INTS] inside d_state.  Two
 *                     descriptors of one table never name the same state: the second would read what the first writes
 *   delay_offset,     int offset of the delay table i32 [channels][table_blocks] inside d_delay; columns [b0, b1) are
 *   table_blocks      written, and the columns the samples use are read
 *   n0, n1            the beamformed samples [n0, n1) the call makes, at the feed's rate
 *   s_first           s_first <= n0: the first sample the destination holds.  [s_first, n0) is COPIED from carry_offset
 *                     (the history a resampler still reads, made by the call before), [n0, n1) is delay-and-sum
 *   dst_offset        float offset of sample s_first inside the destination: [dst_offset, dst_offset + n1 - s_first)
 *   carry_offset      float offset inside d_beam where sample s_first lies, or -1 (then s_first = n0).  The carried range
 *                     and the destination range must not overlap: a call never reads the buffer it writes
 *   src_format,       DZN_SRC_* / 2 .. 64 interleaved channels / the reference channel / the hop, a power of two in
 *   channels, ref,    [256, 4096] / the search range, 1 .. hop / 2, which also bounds the tracked delays / the peak below
 *   hop, max_lag,     which a block's lag is not trusted (float32)
 *   min_peak
 *   dst_space         0: d_pool (a feed at the model's rate: straight into the session's row), 1: d_beam
 *   decode_tile0,     the three tile prefixes (the caller writes them, the call verifies them): tiles owned by the
 *   gcc_item0,        descriptors before this one, where a descriptor owns ceil(src_frames / dzn_beamform_tile()) decode
 *   sum_tile0         tiles, (b1 - b0) * (channels - 1) GCC-PHAT work items and ceil((n1 - s_first) / dzn_beamform_tile())
 *                     sum tiles
 *   reserved          0 */
typedef struct dzn_beamform_desc {
  int64_t src_offset;
  int64_t src_first;
  int64_t src_frames;
  int64_t T;
  int64_t twiddle_offset;
  int64_t planar_offset;
  int64_t ch_stride;
  int64_t lag_offset;
  int64_t blk_cap;
  int64_t b0;
  int64_t b1;
  int64_t seen;
  int64_t state_offset;
  int64_t delay_offset;
  int64_t table_blocks;
  int64_t n0;
  int64_t n1;
  int64_t s_first;
  int64_t dst_offset;
  int64_t carry_offset;
  int32_t src_format;
  int32_t channels;
  int32_t ref;
  int32_t hop;
  int32_t max_lag;
  float min_peak;
  int32_t dst_space;
  int32_t decode_tile0;
  int32_t gcc_item0;
  int32_t sum_tile0;
  int32_t reserved[2];
} dzn_beamform_desc;

/* FOUR launches, enqueue-only, on `hip_stream` of `device` (< 0 = current): no synchronisation, no allocation, no read-back.
 * Every launch is table-driven; a workgroup finds its descriptor by a wave-uniform binary search over the prefix of its launch.
 *   1. the planar decode: one tile of dzn_beamform_tile() frames of one descriptor (dzn_decode_planar's conversions)
 *   2. GCC-PHAT: one workgroup per (descriptor, block, non-reference channel).  Each transforms the reference frame itself and
 *      then its channel's, with the arithmetic of dzn_beamform_delays operation for operation: lag and peak have its bits.
 *      The workgroup of the lowest non-reference channel also writes the reference row's 0 / 0.  Block size and dynamic LDS
 *      are those of the largest hop in the table
 *   3. the tracker: one wavefront per descriptor, a lane per channel (dzn_beamform_track's rule, lags clamped to max_lag)
 *   4. the alignment pass: one tile of dzn_beamform_tile() samples of [s_first, n1) of one descriptor: copied below n0,
 *      dzn_beamform_sum's arithmetic from n0 on
 * so every lag, peak, state, delay and output sample has the bits of dzn_beamform_feed on the same arguments.
 *   d_stage, stage_bytes       the staging buffer on the device and its size
 *   h_desc, d_desc             the table of num_desc descriptors: the host's image (validated here) and the device copy
 *   d_twiddles, twiddle_floats the buffer of twiddle tables and its size in floats
 *   d_planar, planar_floats    the planar scratch
 *   d_lag, d_peak, temp_elems  the lag / peak scratch and its size in elements
 *   d_state, state_ints        the tracker states; d_delay, delay_ints: the delay tables
 *   d_pool, pool_floats        the pooled session buffer; d_beam, beam_floats: the beamformed staging buffers
 * num_desc = 0 launches nothing and returns DZN_OK.  Anything dzn_beamform_feed would refuse for a descriptor's arguments —
 * and b0 != seen, a range that leaves its buffer, a misaligned source, overlapping scratch regions, a tile prefix that is not
 * the prefix, a carried range that overlaps the destination, two descriptors with the same state_offset — makes the WHOLE call
 * return DZN_E_INVALID with a dzn_last_error(NULL) message that names the descriptor index, and launches nothing. */
int dzn_beamform_many(int32_t device, const void* d_stage, int64_t stage_bytes, const dzn_beamform_desc* h_desc,
                      const dzn_beamform_desc* d_desc, int32_t num_desc, const float* d_twiddles, int64_t twiddle_floats,
                      float* d_planar, int64_t planar_floats, int32_t* d_lag, float* d_peak, int64_t temp_elems,
                      int32_t* d_state, int64_t state_ints, int32_t* d_delay, int64_t delay_ints, float* d_pool,
                      int64_t pool_floats, float* d_beam, int64_t beam_floats, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DZN_H_ */
