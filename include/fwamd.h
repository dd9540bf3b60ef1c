/*
 * fwamd.h — C ABI of the MI355X-native Whisper engine (libfwamd.so).
 *
 * This is the drop-in boundary for the hot path of SYSTRAN/faster-whisper:
 * everything the reference reaches through `ctranslate2.models.Whisper`
 * (reference call sites, all in faster_whisper/transcribe.py):
 *
 *   constructor        transcribe.py:689-698   -> fw_model_create / fw_model_free
 *   .is_multilingual   transcribe.py:379,472   -> fw_model_info
 *   .n_mels            transcribe.py:484       -> fw_model_info
 *   .device/.device_index transcribe.py:1394   -> fw_model_info
 *   StorageView.from_array transcribe.py:1875  -> host float* handed to fw_encode
 *   .encode            transcribe.py:1400      -> fw_encode
 *   .generate          transcribe.py:222-236, 1446-1459 -> fw_generate
 *   .detect_language   transcribe.py:215,1193,1823      -> fw_detect_language
 *   .align             transcribe.py:1709-1715          -> fw_align
 *   .score             (not in the reference: CTranslate2's score_batch for Whisper) -> fw_score
 *   boost=             (not in the reference: phrase boosting at the logit) -> fw_boost_create, fw_generate_boost, fw_score_boost
 *   constraint=        (not in the reference: decoding restricted to a phrase list) -> fw_constraint_create,
 *                      fw_generate_constrain, fw_score_constrain
 *
 * plus the log-mel front end the reference runs in numpy on the host
 * (faster_whisper/feature_extractor.py:198-230, called at
 * transcribe.py:463-467 and padded by audio.py:111-123) -> fw_logmel, and a
 * fused PCM -> mel -> encoder entry (fw_encode_pcm) that keeps the features
 * resident in HBM.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types cross this boundary.
 *  - every entry point returns 0 on success, a negative FW_E* code on error;
 *    fw_last_error() returns a thread-local message for the last failure.
 *    The Python shim maps FW_EINVAL -> ValueError, everything else ->
 *    RuntimeError (CTranslate2 surfaces std::invalid_argument / runtime_error
 *    the same way).
 *  - host pointers unless the name says `_dev`.
 *  - the library never falls back to a CPU implementation: without a HIP
 *    device fw_model_create fails with FW_ENODEV.
 */
#ifndef FWAMD_H
#define FWAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_OK 0
#define FW_EINVAL (-1)   /* bad argument / shape (-> ValueError)      */
#define FW_ENODEV (-2)   /* no HIP device / HIP runtime failure       */
#define FW_ENOMEM (-3)   /* device or host allocation failed          */
#define FW_ERUNTIME (-4) /* kernel launch / internal error            */
#define FW_ENOSPC (-5)   /* a caller-provided output buffer is too small (fw_flac_decode): retry with a larger one */

/* 2: fw_model_set_encoder_cus / fw_model_encoder_cus removed, fw_model_set_merge_wait, fw_model_set_decode_lanes and
 *    fw_model_run_capacity added, test / bench hooks moved to fwamd_test.h; the cross-attention cache of a decode group
 *    is one pool shared by its lanes (fw_model_decode_batch = chunks of the pool, fw_model_run_capacity = chunks of one run);
 *    fw_resample_filter and fw_resample_dev were added within version 2 (new symbols only: nothing existing changed),
 *    fw_vad_forward_audio_batch_dev likewise, fw_generate_lp (fw_generate plus per-token log-probabilities) and
 *    fw_score (teacher-forced log-probs of given transcripts), fw_generate_alt (fw_generate_lp plus the n most
 *    likely tokens at every position), fw_boost_create / fw_boost_free / fw_generate_boost / fw_score_boost (phrases made
 *    more likely by a stated amount, at the logit), fw_generate_trunc (top-k / nucleus limits on the sampled draw),
 *    fw_constraint_create / fw_constraint_free / fw_generate_constrain / fw_score_constrain (decoding restricted to a
 *    given phrase list) — new symbols only, each time */
#define FW_ABI_VERSION 2

/* compute types (the reference passes the CTranslate2 strings, transcribe.py:626) */
#define FW_COMPUTE_FLOAT16 0      /* "float16" / "default" on GPU */
#define FW_COMPUTE_INT8_FLOAT16 1 /* "int8_float16": int8 weights + dynamic int8 activations, fp16 elsewhere */

/* weight element types accepted by fw_model_create */
#define FW_DT_F32 0
#define FW_DT_F16 1

#define FW_MAX_ALIGN_HEADS 64

/* Model geometry + vocabulary layout (what CTranslate2 reads from model.bin /
 * config.json). */
typedef struct fw_config {
  int32_t n_mels;         /* 80 or 128 */
  int32_t n_audio_ctx;    /* 1500 */
  int32_t d_model;        /* 384 .. 1280, multiple of 128 */
  int32_t n_heads;        /* d_model / 64 */
  int32_t n_enc_layers;
  int32_t n_dec_layers;
  int32_t n_vocab;        /* 51864 / 51865 / 51866 */
  int32_t n_text_ctx;     /* 448 */
  int32_t is_multilingual;
  /* special token ids */
  int32_t tok_eot, tok_sot, tok_lang_begin, n_langs;
  int32_t tok_translate, tok_transcribe, tok_sot_lm, tok_sot_prev;
  int32_t tok_no_speech, tok_no_timestamps, tok_timestamp_begin;
  /* suppress_blank id set (config.json: suppress_ids_begin): " " token and eot */
  int32_t n_suppress_begin;
  int32_t suppress_begin[8];
  /* alignment heads (config.json: alignment_heads) as (layer, head) pairs;
   * n_align_heads == 0 -> all heads of the upper half of the decoder */
  int32_t n_align_heads;
  int32_t align_heads[2 * FW_MAX_ALIGN_HEADS];
} fw_config;

/* One named weight tensor (names: see faster_whisper_amd/weights.py). */
typedef struct fw_weight {
  const char* name;
  const void* data; /* host pointer, C-contiguous */
  int32_t dtype;    /* FW_DT_* */
  int32_t ndim;
  int64_t dims[4];
} fw_weight;

typedef struct fw_model fw_model;   /* opaque: weights + workspaces on one GPU */
typedef struct fw_tensor fw_tensor; /* opaque: device-resident encoder output [B, n_audio_ctx, d_model] fp16 */

/* generate() options — the kwargs of ctranslate2.models.Whisper.generate that
 * faster-whisper passes (transcribe.py:222-236 and :1433-1459). */
typedef struct fw_gen_opts {
  int32_t beam_size;            /* 1 = greedy */
  float patience;               /* default 1 */
  int32_t num_hypotheses;       /* default 1 */
  float length_penalty;         /* default 1 */
  float repetition_penalty;     /* default 1 (disabled) */
  int32_t no_repeat_ngram_size; /* default 0 (disabled) */
  int32_t max_length;           /* default 448; counts the prompt */
  int32_t return_scores;
  int32_t return_no_speech_prob;
  int32_t max_initial_timestamp_index; /* default 50 */
  int32_t suppress_blank;       /* default 1 */
  const int32_t* suppress_tokens; /* may be NULL; -1 entries are ignored */
  int32_t n_suppress_tokens;
  int32_t sampling_topk;        /* default 1; 0 = full distribution */
  float sampling_temperature;   /* default 1; used only when beam_size==1 and (topk != 1) */
  uint64_t seed;                /* sampling seed (CTranslate2 uses a global seed) */
  /* benchmark-only control (not part of the reference API): when > 0, EOT is
   * suppressed for the first `min_new_tokens` generated tokens, so synthetic
   * weights decode a fixed, input-independent length. */
  int32_t min_new_tokens;
} fw_gen_opts;

const char* fw_last_error(void);
int32_t fw_abi_version(void);

/* Number of visible HIP devices (0 when none / runtime missing). */
int32_t fw_device_count(void);

/* ---- model -------------------------------------------------------------- */
/* Replaces ctranslate2.models.Whisper(...) (transcribe.py:689-698) for ONE
 * device index; the Python shim keeps one fw_model per entry of device_index.
 * Weights are copied to HBM (converted to fp16, or quantised per output row
 * to int8 for FW_COMPUTE_INT8_FLOAT16); the host arrays may be freed after
 * the call returns. max_batch bounds B in every later call (workspaces are
 * allocated once, here). */
int32_t fw_model_create(const fw_config* cfg, const fw_weight* weights, int32_t n_weights,
                        int32_t compute_type, int32_t device_index, int32_t max_batch,
                        int32_t max_beam, fw_model** out);
void fw_model_free(fw_model* m);
int32_t fw_model_info(const fw_model* m, fw_config* cfg_out, int32_t* compute_type,
                      int32_t* device_index, int32_t* max_batch, int32_t* max_beam);
/* Device address / size of a model's weight blob: lets N worker replicas on one GPU share one copy
 * of the weights (CTranslate2's inter_threads / faster-whisper's num_workers, transcribe.py:654-657):
 * create the extra replicas with fw_model_create_from_blob_dev on this pointer.  fw_model_free of the owning
 * model (and of the primary of a decode group) is deferred until its last dependent has been freed. */
int32_t fw_model_blob(const fw_model* m, void** blob_dev, int64_t* blob_bytes);
/* Same model from a weight blob that is ALREADY in HBM on `device_index`
 * (the RCCL-broadcast path: rank 0 packs, ranks receive into device memory).
 * blob layout: faster_whisper_amd/weights.py::pack_blob. */
int32_t fw_model_create_from_blob_dev(const fw_config* cfg, const void* blob_dev, int64_t blob_bytes,
                                      int32_t compute_type, int32_t device_index,
                                      int32_t max_batch, int32_t max_beam, fw_model** out);

/* Decode groups — what CTranslate2's replica pool (inter_threads; transcribe.py:645-657, :689-698) becomes on a
 * GPU with 288 GB of HBM.  A decode step streams every decoder weight once whatever the number of rows, so the
 * worker replicas of a device share ONE decode workspace instead of decoding side by side:
 *   fw_model_set_decode_batch(primary, n_workers * max_batch)  sizes the group for that many chunks in flight: the
 *       cross-attention K / V^T pool holds them (rounded down to whole encoder batches and to what fits in 70 % of the free
 *       HBM; fw_model_decode_batch reads the pool's chunk count back), ONE copy whatever the number of lanes: an encoder
 *       output's block of the pool is handed to whichever lane decodes it.  A decode RUN holds at most
 *       fw_model_run_capacity chunks: 2048 rows with one lane, 1600 rows per lane with two (from four encoder batches on
 *       the group decodes on TWO lanes — two run workspaces, two streams: two decode runs are in flight at once, the
 *       HBM-bound cross-attention of one beside the linears of the other).  The self-attention cache of a lane is rows x
 *       positions and every run lays it out for its own max_length, so a run of calls with a short max_length holds more
 *       chunks than one that asks for the whole text context (positions per row are lowered, down to 160, before the
 *       pool is).  Setup-time call: FW_EINVAL while the group has decode runs queued or in flight; fw_generate calls that
 *       arrive during the rebuild wait for it;
 *   fw_model_join_decoder(worker, primary)  frees the worker's own decode workspace and routes its fw_generate /
 *       fw_detect_language / fw_align calls to the primary's.
 * fw_generate calls that arrive from different host threads while a decode run is in progress are merged into the
 * next run (up to decode_batch chunks); each caller gets exactly the result it would get alone.  What must agree for two
 * calls to share a run: beam_size, patience, num_hypotheses, length_penalty, repetition_penalty, no_repeat_ngram_size,
 * max_length, max_initial_timestamp_index, suppress_blank, min_new_tokens, the suppress list, the boost list
 * (fw_generate_boost: none on both sides, or byte-equal compiled tables), the constraint list (fw_generate_constrain: the
 * same rule), and the timestamp mode
 * (<|notimestamps|> in the prompt or not).  Sampling calls (beam_size 1, sampling_topk 0) merge among themselves, never with
 * beam or greedy calls; their sampling_temperature and seed need NOT agree (every row of a run draws with its own call's,
 * as the row of that call that it is alone), and neither do the top_k / top_p of fw_generate_trunc (a truncating call
 * shares runs with sampling calls that truncate otherwise or not at all).  The PROMPT LENGTH and the position of
 * <|startoftranscript|> need NOT agree: every chunk of a run decodes at its own position of the text context with its
 * own budget min(max_length, n_text_ctx) - prompt length (so prompts that carry different amounts of previous text
 * share a run; only a call whose prompt already fills max_length keeps to calls of its own prompt length).  Inside ONE
 * call all prompts must still have the same length (FW_EINVAL).  Encoders keep running per worker on their own streams
 * and overlap with the running decode. */
int32_t fw_model_set_decode_batch(fw_model* m, int32_t decode_batch);
int32_t fw_model_decode_batch(const fw_model* m);
/* chunks one decode run of the group can hold (<= fw_model_decode_batch) */
int32_t fw_model_run_capacity(const fw_model* m);
int32_t fw_model_join_decoder(fw_model* worker, fw_model* primary);
/* How long, and for how much, the leader of a decode run waits for the requests of workers that are still encoding
 * (latency of the waiting call against rows per run).  wait_ms: -1 = 2.5 measured encoder passes after the last arrival,
 * at most 250 ms (default); 0 = never wait (every call starts its run at once: lowest latency); n > 0 = n milliseconds.
 * fill_percent: the leader stops waiting once that share of a run's chunk capacity is queued (default 90: large runs
 * amortise the decoder weights and launches over more rows and take the GEMM-shaped decoder linears; measured 2 917x
 * at 50, 2 965x at 75, 2 975x at 95; smaller = lower latency).  It never waits when no member encode is in flight.  A group with NO run in progress and two
 * lanes leads earlier: it splits the work it knows of (queued requests + one per worker inside an encode call) evenly over
 * the runs that work needs — 20 batches in flight become two runs of 10 instead of one of 18 after 18 serial encoder
 * passes and leftovers (FWAMD_IDLE_BALANCE=0 restores the plain rule). */
int32_t fw_model_set_merge_wait(fw_model* m, int32_t wait_ms, int32_t fill_percent);
/* Decode runs the group may have in flight: 2 (default, when the group has two lanes) or 1 (one run at a time: every
 * kernel of a run has the chip to itself — what per-kernel timing wants; takes effect with the next run).  A group built
 * with FWAMD_DECODE_LANES = 3 / 4 in the environment (measurement knob) has that many lanes and takes 1 .. that many. */
int32_t fw_model_set_decode_lanes(fw_model* m, int32_t lanes);
/* counters of the decode group `m` belongs to: decode runs, fw_generate calls served, chunks decoded, chunks of
 * the largest run (any pointer may be NULL) */
int32_t fw_model_decode_stats(const fw_model* m, int64_t* runs, int64_t* requests, int64_t* chunks,
                              int32_t* max_run_chunks);

/* Host image of the device weight blob (what rank 0 broadcasts over RCCL/xGMI at load):
 * fw_pack_blob_size packs and returns a handle + byte size, fw_pack_blob_copy copies the
 * image into caller memory, fw_pack_blob_free releases the handle. */
int32_t fw_pack_blob_size(const fw_config* cfg, const fw_weight* weights, int32_t n_weights,
                          int32_t compute_type, int64_t* size_out, void** handle_out);
int32_t fw_pack_blob_copy(void* handle, void* dst, int64_t dst_bytes);
void fw_pack_blob_free(void* handle);

/* ---- log-mel front end ---------------------------------------------------
 * FeatureExtractor.__call__(chunk)[..., :-1] followed by pad_or_trim(., 3000)
 * for B ragged chunks (feature_extractor.py:198-230, transcribe.py:463-467,
 * 514-516, audio.py:111-123). pcm: the B chunks back to back; offsets[B+1]
 * sample offsets into pcm (chunk b = pcm[offsets[b] .. offsets[b+1])).
 * out: float32 [B, n_mels, 3000]. n_frames_out (may be NULL): frames that
 * carry signal per chunk (min(3000, n_b/160)). */
int32_t fw_logmel(fw_model* m, const float* pcm, const int64_t* offsets, int32_t B,
                  float* out, int32_t* n_frames_out);
/* Whole-waveform variant used by the sequential path and detect_language:
 * FeatureExtractor.__call__(waveform) without the trailing-frame drop and
 * without pad_or_trim (transcribe.py:916). out: [n_mels, n_samples/160 + 1]. */
int32_t fw_logmel_full(fw_model* m, const float* pcm, int64_t n_samples, float* out, int64_t out_frames);

/* ---- encoder -------------------------------------------------------------
 * ctranslate2.models.Whisper.encode (transcribe.py:1400): features float32
 * [B, n_mels, 3000] on the host -> device-resident encoder output handle. */
int32_t fw_encode(fw_model* m, const float* features, int32_t B, fw_tensor** out);
/* Fused resident path: ragged PCM -> log-mel -> encoder without the features
 * ever leaving HBM (same numerics as fw_logmel + fw_encode). */
int32_t fw_encode_pcm(fw_model* m, const float* pcm, const int64_t* offsets, int32_t B, fw_tensor** out);
/* As fw_encode_pcm, but pcm_dev already resides in HBM (bench.py: inputs are
 * resident when the timed region starts). */
int32_t fw_encode_pcm_dev(fw_model* m, const float* pcm_dev, const int64_t* offsets, int32_t B, fw_tensor** out);
int32_t fw_tensor_shape(const fw_tensor* t, int32_t* B, int32_t* T, int32_t* D);
/* encoder output as float32 [B, T, D] on the host (StorageView -> numpy; to_cpu=True) */
int32_t fw_tensor_to_host(fw_model* m, const fw_tensor* t, float* out);
/* upload a host float32 [B, T, D] encoder output (the to_cpu round trip, transcribe.py:1392-1394) */
int32_t fw_tensor_from_host(fw_model* m, const float* data, int32_t B, fw_tensor** out);
void fw_tensor_free(fw_tensor* t);

/* ---- generate ------------------------------------------------------------
 * ctranslate2.models.Whisper.generate. prompts: B prompts back to back,
 * prompt_offsets[B+1]. Outputs, per chunk b and hypothesis h < num_hypotheses:
 *   out_ids    int32 [B, num_hypotheses, max_length]  generated ids (no prompt, no eot)
 *   out_lens   int32 [B, num_hypotheses]
 *   out_scores float [B, num_hypotheses]  cum_logprob / len^length_penalty (0 if !return_scores)
 *   out_no_speech float [B]               (0 if !return_no_speech_prob)
 */
int32_t fw_generate(fw_model* m, const fw_tensor* enc, const int32_t* prompts,
                    const int32_t* prompt_offsets, int32_t B, const fw_gen_opts* opts,
                    int32_t* out_ids, int32_t* out_lens, float* out_scores, float* out_no_speech);
/* fw_generate, plus per-token log-probabilities of every returned hypothesis:
 *   out_token_logprobs float [B, num_hypotheses, max_length]  entry t = log-prob (after the logits rules, fp32 log-softmax)
 *                                                             of out_ids[..., t]; entries >= out_lens are 0
 *   out_end_logprobs   float [B, num_hypotheses]              log-prob of the <eot> that closed the hypothesis, 0 when it
 *                                                             was cut at the budget
 * Either pointer may be NULL.  Adding the values of a hypothesis in order in float32, then the end value, reproduces
 * the cumulative log-prob that out_scores normalises — exactly.  These are the log-probs of the PROCESSED distribution,
 * the one the search itself ranks by: after the repetition penalty, the no-repeat n-gram, suppress and timestamp rules
 * (a token the rules left alone on a row gets log-prob 0).  When sampling they are not tempered.  fw_align's
 * text_token_probs are the unconstrained counterpart: a second decoder pass without the rules.  fw_generate is
 * fw_generate_lp(..., NULL, NULL); a call that asks for log-probs shares decode runs with calls that do not. */
int32_t fw_generate_lp(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets, int32_t B,
                       const fw_gen_opts* opts, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                       float* out_no_speech, float* out_token_logprobs, float* out_end_logprobs);
/* fw_generate_lp, plus the n_alt most likely tokens at every position of every returned hypothesis: what else the model
 * considered there, and how close it was.
 *   out_alt_ids / out_alt_logprobs          int32 / float [B, num_hypotheses, max_length, n_alt]
 *   out_end_alt_ids / out_end_alt_logprobs  int32 / float [B, num_hypotheses, n_alt]
 * Entry [b, h, t, :] holds the n_alt most likely ids, with their log-probs, of the distribution out_ids[b, h, t] was
 * chosen from: the one on the hypothesis's own row at that step, and the one out_token_logprobs speaks of (after the
 * repetition penalty, the n-gram, suppress and timestamp rules, fp32 log-softmax, not tempered when sampling).  The end
 * arrays hold the same for the step that produced the closing <eot>.  Order: log-prob descending, id ascending.  A
 * distribution with fewer than n_alt live ids fills the tail with (id 0, -inf).  Entries at t >= out_lens are (id -1,
 * log-prob 0), and so are the end entries of a hypothesis that was cut at the budget (it has no closing step): the id -1
 * is the mark, a genuine log-prob can be 0.
 * Two identities hold exactly: (1) when out_ids[b, h, t] is among the alternatives of its position, its log-prob there is
 * out_token_logprobs[b, h, t] bit for bit (when it is not, out_token_logprobs[b, h, t] <= the last alternative's), and
 * likewise <eot> and out_end_logprobs; for a greedy call alternative 0 IS (out_ids, out_token_logprobs).  (2) fw_score
 * with the call's rules on out_ids[b, h, :t] followed by an alternative id returns that alternative's log-prob bit for
 * bit for a greedy hypothesis, and its out_best_ids at that position is alternative 0.
 * 0 <= n_alt <= FW_MAX_ALTERNATIVES.  n_alt == 0 requires the four pointers to be NULL and is fw_generate_lp; n_alt > 0
 * requires all four.  Anything else is FW_EINVAL before anything is queued.  A call with alternatives shares decode runs
 * with calls without and with calls of another n_alt, and every caller gets what it would get alone, bit for bit.  The
 * buffers behind this are allocated by the first decode run that needs them (FW_ENOMEM for the calls of that run). */
#define FW_MAX_ALTERNATIVES 8
int32_t fw_generate_alt(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                        int32_t B, const fw_gen_opts* opts, int32_t n_alt,
                        int32_t* out_ids, int32_t* out_lens, float* out_scores, float* out_no_speech,
                        float* out_token_logprobs, float* out_end_logprobs,
                        int32_t* out_alt_ids, float* out_alt_logprobs,          /* [B, num_hypotheses, max_length, n_alt] */
                        int32_t* out_end_alt_ids, float* out_end_alt_logprobs); /* [B, num_hypotheses, n_alt] */

/* ---- phrase boosting (contextual biasing; not in CTranslate2) ----------------
 * A boost list is n_phrases phrases.  Phrase j is the token-id sequence p_j[0 .. L_j) = tokens[offsets[j] .. offsets[j + 1])
 * with one float boosts[j].  Consider a row whose GENERATED history is h[0 .. n) (generated tokens only, timestamps
 * included, never the prompt).  The pair (j, k), 0 <= k < L_j, MATCHES when k <= n and h[n - k .. n) == p_j[0 .. k); k = 0
 * always matches, so a phrase's first token is boosted at every step.  The boost of an id v is the MAXIMUM boosts[j] over
 * all matching pairs with p_j[k] == v — a max, never a sum: phrase [a, a, a] after history [a, a] boosts `a` once — and
 * logit[v] += boost(v) is one fp32 add.  Ids with no matching pair keep their bits.
 * The boost comes FIRST; the rules then run exactly as always (repetition penalty, no-repeat n-gram, suppress, timestamp
 * rules, log-softmax).  So the rules still win (a forbidden id stays -inf), token log-probs, alternatives and scores are
 * those of the boosted, processed distribution, and sampling draws from it.  There is no back-off (nothing is subtracted
 * when a match breaks) and no matching across the prompt boundary.
 * fw_boost_create is host code: it needs no device and no model.  It validates the list and compiles it into the table the
 * kernel walks (entries (j, k) grouped by target id: one worker owns one id and does one add).  FW_EINVAL: n_vocab < 1, a
 * null pointer with n_phrases > 0, more than FW_BOOST_MAX_PHRASES phrases, offsets[0] != 0, a phrase of no token or of more
 * than FW_BOOST_MAX_LEN, more than FW_BOOST_MAX_TOKENS tokens in all, an id outside [0, n_vocab), a boost that is not
 * finite.  An empty list (n_phrases == 0; the pointers may be NULL) is valid and does nothing. */
#define FW_BOOST_MAX_PHRASES 1024
#define FW_BOOST_MAX_LEN 32
#define FW_BOOST_MAX_TOKENS 4096
typedef struct fw_boost fw_boost;   /* opaque: a validated, compiled boost list (host memory); any number of calls may read it at once */
int32_t fw_boost_create(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
                        const float* boosts, fw_boost** out);
void fw_boost_free(fw_boost* b);
/* fw_generate_alt plus a boost list.  boost == NULL (or an empty list) is fw_generate_alt exactly; FW_EINVAL when the list
 * was built for another n_vocab than the model's.  Identity (1) of fw_generate_alt holds unchanged on boosted calls, and
 * (2) with fw_score_boost in fw_score's place.  Two calls share a decode run only when both have no list or their compiled
 * tables are byte-equal (lists built separately from equal arguments are): a boosted call never shares a run with a plain
 * one; everything else about merging is unchanged, and every caller gets its solo result bit for bit.  A boosted run costs
 * one small kernel launch per step more; its table is copied into a buffer of the decode lane at the start of the run
 * (the list may be freed once the call has returned). */
int32_t fw_generate_boost(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                          int32_t B, const fw_gen_opts* opts, int32_t n_alt, const fw_boost* boost,
                          int32_t* out_ids, int32_t* out_lens, float* out_scores, float* out_no_speech,
                          float* out_token_logprobs, float* out_end_logprobs,
                          int32_t* out_alt_ids, float* out_alt_logprobs,
                          int32_t* out_end_alt_ids, float* out_end_alt_logprobs);

/* ---- truncated sampling: top-k and nucleus (top-p) limits on the sampled draw -------------------------------
 * fw_generate_boost plus two limits on what a SAMPLING call (beam_size 1, sampling_topk 0) may draw.  For one row at one
 * step, after the boost, the rules and the fp32 log-softmax exactly as always, with logp[v] the processed log-prob:
 *   1. L = {v : logp[v] > -inf}, in the order of the alternatives: logp descending, id ascending.
 *   2. top-k: S_k = the first min(top_k, |L|) ids of L (ties at the cut go to the lower id); S_k = L when top_k == 0.
 *   3. nucleus: w(v) = exp((logp[v] - max logp) / sampling_temperature) — temperature comes before the nucleus —, Z = the
 *      sum of w over S_k, S = {v in S_k : the sum of w over the ids of S_k in front of v is < top_p * Z}; S = S_k when
 *      top_p == 1.  The first id of the order is always in S.  The sums are fp32 in an order of the implementation's: an id
 *      whose mass-ahead lies within rounding of top_p * Z may fall on either side.
 *   4. the draw is the arg-max over S of logp[v] / T + gumbel(seed, row, step, v), lowest id on a tie.  The noise of an id
 *      does not depend on S: whenever the untruncated draw lies in S, the truncated draw is that same id.
 *   5. what is recorded does not change: out_token_logprobs is the plain processed logp of the drawn id (not tempered, not
 *      renormalised over S), the alternatives are the plain top n_alt of L, and identities (1) and (2) of fw_generate_alt
 *      hold as they are.
 * top_k == 0 && top_p == 1 is fw_generate_boost exactly, bit for bit.  top_k == 1 draws the arg-max: ids and token
 * log-probs of a one-hypothesis call equal the greedy call's.  FW_EINVAL before anything is queued: top_k < 0; top_p NaN,
 * <= 0 or > 1; a limit (top_k > 0 or top_p < 1) on a call that does not sample.  opts->sampling_topk keeps its meaning
 * (1 greedy, 0 sample; anything else FW_EINVAL).
 * Merging: top_k and top_p need NOT agree — like temperature and seed they are per call and travel in a per-row table.  A
 * truncating call shares decode runs with other sampling calls, truncating or not, and every caller gets its solo result
 * bit for bit; a run with no truncating call launches the kernels and graphs it always did.
 * [CT2-ext] CTranslate2's own sampler (sampling_topk > 1, sampling_topp) is not reached by the reference and is not on hand:
 * whether it renormalises in exactly this order (temperature, top-k, then the nucleus over the top-k mass) is not pinned,
 * next to the A.7 unknowns of SURVEY.md. */
int32_t fw_generate_trunc(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                          int32_t B, const fw_gen_opts* opts, int32_t top_k, float top_p, int32_t n_alt,
                          const fw_boost* boost,
                          int32_t* out_ids, int32_t* out_lens, float* out_scores, float* out_no_speech,
                          float* out_token_logprobs, float* out_end_logprobs,
                          int32_t* out_alt_ids, float* out_alt_logprobs,
                          int32_t* out_end_alt_ids, float* out_end_alt_logprobs);

/* ---- constrained decoding: the transcript is one of a given phrase list (not in CTranslate2) ----------------
 * The counterpart of the boost: a boost adds in front of the rules, a constraint REMOVES in front of the rules.  A
 * constraint list is n_phrases phrases of token ids, laid out as a boost list (tokens, offsets) under limits of its own,
 * without floats.  Phrase j is p_j[0 .. L_j).  For one logits row let h[0 .. n) be the row's GENERATED history (never the
 * prompt) and t[0 .. m) be h without its ids >= tok_timestamp_begin.  Then
 *   M = {j : m <= L_j and p_j[0 .. m) == t},  A = {p_j[m] : j in M, m < L_j},  <eot> is allowed iff some j in M has L_j == m.
 * What is written, and nothing else:
 *   - every id v < tok_timestamp_begin keeps its bits if it is in A, or if it is <eot> and <eot> is allowed; otherwise
 *     logit[v] = -inf;
 *   - the ids >= tok_timestamp_begin keep their bits when the timestamp rules are on (no <|notimestamps|> in the prompt);
 *     with <|notimestamps|> they become -inf;
 *   - nothing is added to any logit.
 * A history that is a prefix of no phrase has M empty: no text id and no <eot>.  In fw_generate_constrain that arises on
 * dead beam copies only; in scoring it is a target that left the list, which gets -inf from there on.
 * Order per step: the boost if there is one, then the constraint, then the rules exactly as always.  Token log-probs,
 * alternatives, scores and sampled draws are those of the constrained, processed distribution; a position with fewer live
 * ids than n_alt fills the tail with (0, -inf) as documented at fw_generate_alt.  out_no_speech is unaffected (it is read
 * before the rules).
 * THE GUARANTEE: take a returned hypothesis with a finite score and remove its timestamp ids.  If it closed on <eot>, what
 * remains is a phrase of the list; if it was cut at the budget, what remains is a prefix of a phrase: a proper one,
 * except where the budget ended on the very step that would have closed a whole phrase with <eot>.
 * OUT OF SCOPE: a SEQUENCE of phrases (a repeat mode needs per-row automaton state or a prefix-free list), grammars, and
 * different lists for the calls of one run (a run walks one table).
 * fw_constraint_create is host code: it needs no device and no model.  FW_EINVAL: n_vocab < 1, a null pointer with
 * n_phrases > 0, more than FW_CONSTRAIN_MAX_PHRASES phrases, offsets[0] != 0, a phrase of no token or of more than
 * FW_CONSTRAIN_MAX_LEN, more than FW_CONSTRAIN_MAX_TOKENS tokens in all, an id outside [0, n_vocab).  Duplicate phrases
 * are valid, and so is a phrase that is a prefix of another (<eot> and the longer phrase's next token are then both
 * allowed).  An empty list (n_phrases == 0; the pointers may be NULL) is valid and means NO constraint, as with the boost.
 * The list compiles to one int32 table: the phrases as a set, sorted by their ids, duplicates dropped.  Equal arguments
 * give byte-equal tables, and so do lists that name the same phrases in another order or more than once. */
#define FW_CONSTRAIN_MAX_PHRASES 1024
#define FW_CONSTRAIN_MAX_LEN 32
#define FW_CONSTRAIN_MAX_TOKENS 4096
typedef struct fw_constraint fw_constraint;   /* opaque: a validated, compiled list (host memory); any number of calls may read it at once */
int32_t fw_constraint_create(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
                             fw_constraint** out);
void fw_constraint_free(fw_constraint* c);
/* fw_generate_trunc plus a constraint list.  constraint == NULL (or an empty list) is fw_generate_trunc exactly, bit for
 * bit.  FW_EINVAL before anything is queued, each message naming the phrase (the caller's index) and the id:
 *   - the list was built for another n_vocab than the model's;
 *   - a phrase id is >= tok_eot (phrases are text);
 *   - a phrase id is in opts' suppress list;
 *   - opts->suppress_blank is set and a phrase's first id is one of the model's suppress_begin ids;
 *   - opts->no_repeat_ngram_size > 0;
 *   - opts->min_new_tokens > 0.
 * The last four would make a listed phrase unreachable or leave a row without a live id.
 * Merging: two calls share a decode run only when both have no list or their compiled tables are byte-equal — the rule of
 * the boost list, beside it; a constrained call never shares a run with a plain one, and every caller gets its solo result
 * bit for bit.  A constrained run costs one kernel launch per step more (it writes -inf over rows x n_vocab floats); its
 * table is copied into a buffer of the decode lane at the start of the run (the list may be freed once the call has
 * returned).  Identity (1) of fw_generate_alt holds unchanged, and (2) with fw_score_constrain in fw_score's place. */
int32_t fw_generate_constrain(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                              int32_t B, const fw_gen_opts* opts, int32_t top_k, float top_p, int32_t n_alt,
                              const fw_boost* boost, const fw_constraint* constraint,
                              int32_t* out_ids, int32_t* out_lens, float* out_scores, float* out_no_speech,
                              float* out_token_logprobs, float* out_end_logprobs,
                              int32_t* out_alt_ids, float* out_alt_logprobs,
                              int32_t* out_end_alt_ids, float* out_end_alt_logprobs);

/* ---- score ---------------------------------------------------------------
 * Teacher-forced log-probs of GIVEN transcripts (CTranslate2 has score_batch for its other model classes): how likely
 * is this text under the model, for text that was not decoded here — a corrected transcript, another system's output,
 * an n-best list.  prompts: B prompts of equal length, as fw_generate.  targets: B * H sequences back to back,
 * target_offsets[B * H + 1], ragged, any of them may be empty; sequence i = b * H + h is candidate h of chunk b of `enc`
 * (1 <= H <= max_beam: the candidates of a chunk share its cross-attention K/V the way beams do).
 * Outputs, three arrays of target_offsets[B * H] + B * H entries: sequence i with n_i targets owns entries
 * target_offsets[i] + i .. + n_i of each; the first n_i belong to its tokens, the last to the <eot> that would close it.
 *   out_token_logprobs  log-prob of the given token (of <eot> in the last entry); -inf for a token the rules forbid
 *   out_best_ids        the arg-max of the same distribution (ties: the lowest id) ...
 *   out_best_logprobs   ... and its log-prob.  Both NULL, or both given.
 * rules == NULL: the raw distribution (fp32 log-softmax of the logits).  Otherwise the distribution fw_generate's search
 * ranks by, for a greedy row whose history is the sequence's own prefix: repetition_penalty, no_repeat_ngram_size,
 * suppress_blank, suppress_tokens and max_initial_timestamp_index are read, the timestamp rules are on unless the prompts
 * carry <|notimestamps|> (they must agree on it), and EVERY other field — beam_size, patience, num_hypotheses,
 * length_penalty, max_length, min_new_tokens, the return_* switches, sampling_* and seed — is ignored.  Adding a
 * sequence's entries in order in float32 then gives the cumulative log-prob fw_generate would normalise into its score.
 * FW_EINVAL before anything is launched: a null argument, B != the encoder output's batch or > max_batch, H out of range,
 * an id outside [0, n_vocab), prompt length + n_i + 1 > n_text_ctx, offsets that decrease, more rows than a decode lane
 * holds.  Runs on the first decode lane like fw_align: prompt + targets go through the decoder in position blocks, one
 * scoring-kernel launch per block. */
int32_t fw_score(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                 const int32_t* targets, const int32_t* target_offsets, int32_t B, int32_t H, const fw_gen_opts* rules,
                 float* out_token_logprobs, int32_t* out_best_ids, float* out_best_logprobs);
/* fw_score plus a boost list (above): the boost is added to every scored row's logits first, with the row's history —
 * the sequence's own prefix — as the generated history, then the rules run.  boost == NULL (or an empty list) is fw_score
 * exactly; boost != NULL needs rules != NULL (FW_EINVAL), and a list built for the model's n_vocab (FW_EINVAL).  For a
 * greedy hypothesis of fw_generate_boost, fw_score_boost with the call's rules and list returns its out_token_logprobs
 * and out_end_logprobs bit for bit, and out_best_ids / out_best_logprobs are its alternative 0. */
int32_t fw_score_boost(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                       const int32_t* targets, const int32_t* target_offsets, int32_t B, int32_t H, const fw_gen_opts* rules,
                       const fw_boost* boost, float* out_token_logprobs, int32_t* out_best_ids, float* out_best_logprobs);
/* fw_score_boost plus a constraint list (constrained decoding, above): on every scored row the boost (if any), then the
 * constraint with the sequence's own prefix as the generated history, then the rules.  constraint == NULL (or an empty
 * list) is fw_score_boost exactly; otherwise rules != NULL is needed, and the checks of fw_generate_constrain run against
 * the rules' fields (FW_EINVAL; min_new_tokens is not read by scoring and not checked).  A target sequence that leaves the
 * list at position q scores finite before q and -inf from q on, its <eot> entry included.  For a greedy hypothesis of
 * fw_generate_constrain it returns out_token_logprobs and out_end_logprobs bit for bit, and out_best_ids /
 * out_best_logprobs are its alternative 0.  Re-recognition against an n-best list larger than max_beam: one constrained
 * generate call instead of ceil(n / max_beam) scoring calls. */
int32_t fw_score_constrain(fw_model* m, const fw_tensor* enc, const int32_t* prompts, const int32_t* prompt_offsets,
                           const int32_t* targets, const int32_t* target_offsets, int32_t B, int32_t H,
                           const fw_gen_opts* rules, const fw_boost* boost, const fw_constraint* constraint,
                           float* out_token_logprobs, int32_t* out_best_ids, float* out_best_logprobs);

/* ---- detect_language -------------------------------------------------------
 * ctranslate2.models.Whisper.detect_language: one decoder step on [sot];
 * softmax restricted to the language ids. out_lang_ids / out_probs:
 * [B, n_langs], sorted by descending probability. */
int32_t fw_detect_language(fw_model* m, const fw_tensor* enc, int32_t B,
                           int32_t* out_lang_ids, float* out_probs);

/* ---- align -----------------------------------------------------------------
 * ctranslate2.models.Whisper.align (transcribe.py:1709-1715).
 * start_seq[n_start]: sot sequence; text tokens ragged via text_offsets[B+1];
 * num_frames[B] (mel frames, the reference passes segment_size).
 * Outputs: out_pairs int32 [B, max_pairs, 2] (text_idx, time_idx) with
 * out_n_pairs[B]; out_probs float ragged like text tokens (same offsets).
 * text_idx runs over n_text + 1 rows: row 0 is the <|notimestamps|> position
 * (its attention times the first text token), row n_text the last text token;
 * the reference looks the path's token jumps up with word boundaries 0..n_text
 * (transcribe.py:1741-1745).  time_idx < num_frames / 2.
 * max_pairs >= n_text + 1 + num_frames / 2. */
int32_t fw_align(fw_model* m, const fw_tensor* enc, const int32_t* start_seq, int32_t n_start,
                 const int32_t* text_tokens, const int32_t* text_offsets, const int32_t* num_frames,
                 int32_t B, int32_t median_filter_width, int32_t max_pairs,
                 int32_t* out_pairs, int32_t* out_n_pairs, float* out_probs);

/* ---- measurement hooks (bench.py) ------------------------------------------
 * Per-kernel-family GPU time accumulated with HIP events on the engine's own
 * stream while profiling is enabled. names: fw_prof_name(i), i < fw_prof_count(). */
void fw_prof_enable(fw_model* m, int32_t on);
void fw_prof_reset(fw_model* m);
int32_t fw_prof_count(void);
const char* fw_prof_name(int32_t i);
/* total ms, launches, algorithmic flops, algorithmic bytes for family i */
int32_t fw_prof_get(fw_model* m, int32_t i, double* ms, int64_t* launches, double* flops, double* bytes);
/* block until all work queued on the model's streams has finished */
int32_t fw_synchronize(fw_model* m);
/* raw device allocation helpers so bench.py can stage PCM in HBM without torch */
int32_t fw_dev_alloc(fw_model* m, int64_t bytes, void** out_dev);
int32_t fw_dev_free(fw_model* m, void* dev);
int32_t fw_dev_upload(fw_model* m, void* dst_dev, const void* src_host, int64_t bytes);

/* ---- Silero VAD network (host) ----------------------------------------------
 * Replaces the reference's SileroVADModel (faster_whisper/vad.py:295-351: onnxruntime on the CPU, one thread,
 * asset silero_vad_v6.onnx).  Host C++: needs no GPU.  The weights are the initializers of that ONNX file, passed
 * as plain float32 arrays (faster_whisper_amd/onnx_lite.py reads them); the architecture is fixed to Silero v6:
 *   stft_basis [258][256]; conv_w {[128][129][3], [64][128][3], [64][64][3], [128][64][3]} + conv_b;
 *   lstm_w / lstm_r [512][128] in ONNX gate order i,o,f,c; lstm_b [1024] = Wb | Rb; dec_w [128], dec_b.
 * fw_vad_forward: windows [n][576] float32 (64 samples of context + 512 new samples each, exactly what
 * SileroVADModel.__call__ feeds the session, vad.py:318-336); h, c [128] LSTM state, updated in place (the
 * windows are the LSTM's sequence; the reference carries h / c across its batches of 10 000 windows);
 * probs [n] speech probability per window.  n_threads <= 0: all host cores. */
typedef struct fw_vad fw_vad;
typedef struct fw_vad_weights {
  const float* stft_basis;
  const float* conv_w[4];
  const float* conv_b[4];
  const float* lstm_w;
  const float* lstm_r;
  const float* lstm_b;
  const float* dec_w;
  float dec_b;
} fw_vad_weights;
int32_t fw_vad_create(const fw_vad_weights* w, fw_vad** out);
int32_t fw_vad_forward(fw_vad* v, const float* windows, int64_t n, int32_t n_threads, float* h, float* c,
                       float* probs);
void fw_vad_free(fw_vad* v);
/* Same computation on HIP device `device_index` (csrc/vad.hip: one workgroup per window for the front end, one
 * persistent workgroup for the LSTM recurrence); host pointers in and out.  Checked on hardware against the host
 * path and against the numpy restatement of the ONNX graph (tests/test_gpu_vad.py); the Python front uses the host
 * path by default (the reference runs the VAD on the CPU, vad.py:295-351). */
int32_t fw_vad_forward_dev(fw_vad* v, int32_t device_index, const float* windows, int64_t n, float* h, float* c,
                           float* probs);
/* The same network over a whole RECORDING: `audio` = n_samples float32 samples in host memory, n_samples a multiple of 512
 * (the reference pads with 1..512 zeros, vad.py:79-81); the 576-sample rows [64 context | 512 window] the network takes are
 * formed on the device exactly as SileroVADModel.__call__ forms them on the host (faster_whisper/vad.py:318-336: context
 * = tail of the previous window, zeros for the first; the last 64 samples of the last window zeroed), so no [n][576] copy
 * of the recording is built or transferred.  probs: n_samples / 512 values. */
int32_t fw_vad_forward_audio_dev(fw_vad* v, int32_t device_index, const float* audio, int64_t n_samples, float* h, float* c,
                                 float* probs);
/* N recordings in one device call.  audio: the recordings back to back, each padded to a multiple of 512 samples
 * (as fw_vad_forward_audio_dev takes ONE); offsets[n_rec + 1]: sample offsets, non-decreasing, multiples of 512
 * (an empty recording is allowed);  h, c: [n_rec][128] LSTM states, updated in place per recording;
 * probs: offsets[n_rec] / 512 values, recording after recording.
 * Recording r's probabilities and final h / c are bit for bit those of fw_vad_forward_audio_dev on that recording alone:
 * the front end is ONE launch over the windows of all recordings (a workgroup finds its recording in a device table of
 * first windows and frames per recording: zero context for a recording's first window, the last 64 samples of its last
 * window zeroed), the recurrence one workgroup PER RECORDING, all launched together, so N recordings cost about the time
 * of the longest one.  One set of device buffers per call.  The recordings are processed in groups of consecutive
 * recordings of at most FW_VAD_BATCH_MAX_WINDOWS windows in total: the gate pre-activations of a group are 2 KB per
 * window, so 131 072 windows (70 min of audio) bound that buffer at 256 MiB — no more than the single call allocates for
 * a 70-minute recording — and a group of that size is already 131 072 front-end workgroups, far more than the device
 * holds at once; a single recording above the bound forms a group of its own, as fw_vad_forward_audio_dev runs it.
 * FW_EINVAL: n_rec < 0, a null pointer, offsets that decrease, are negative or are no multiple of 512 (nothing is started
 * on the device); FW_ENODEV: no such device; n_rec == 0: FW_OK. */
#define FW_VAD_BATCH_MAX_WINDOWS 131072
int32_t fw_vad_forward_audio_batch_dev(fw_vad* v, int32_t device_index, const float* audio, const int64_t* offsets,
                                       int32_t n_rec, float* h, float* c, float* probs);

/* ---- audio front: native FLAC decoding --------------------------------------------
 * The reference decodes every container through PyAV / FFmpeg (faster_whisper/audio.py:19-76); its own test asset
 * (tests/data/jfk.flac) is FLAC.  fw_flac_info reads STREAMINFO (total_samples is per channel, 0 = unknown);
 * fw_flac_decode decodes the whole stream (host code, csrc/flac_host.cpp) into interleaved int32 samples
 * out[sample][channel] (capacity_samples per channel), verifying every frame's CRC-8 / CRC-16, and reports in md5_status
 * whether the decoded PCM carries the MD5 signature the encoder stored: 1 = yes (bit-exact decode), 0 = no, -1 = nothing
 * to compare with (no signature, or a truncated stream: the whole frames present are returned).
 * FW_ENOSPC: the stream holds more than capacity_samples per channel (nothing usable was written): retry with a larger buffer. */
int32_t fw_flac_info(const uint8_t* data, int64_t n_bytes, int32_t* sample_rate, int32_t* channels,
                     int32_t* bits_per_sample, int64_t* total_samples);
int32_t fw_flac_decode(const uint8_t* data, int64_t n_bytes, int32_t* out, int64_t capacity_samples,
                       int64_t* n_decoded, int32_t* md5_status);

/* ---- audio front: sample-rate conversion on the device (csrc/resample.hip) ---------------------------------------
 * The Kaiser-windowed-sinc polyphase converter of faster_whisper_amd/audio.py::resample (the reference resamples inside
 * PyAV / libswresample, faster_whisper/audio.py:42-62).  g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g,
 * big = max(up, down), half = taps_per_phase * big / 2; prototype h[t], t = -half .. half: 2c sinc(2c t) kaiser(beta) with
 * c = 0.5 / big, scaled to sum up; y[m] = sum_k h[half + k up - m down] x[k], x zero outside [0, n).  float32 samples,
 * fp64 coefficients and accumulation.  No fw_model is needed. */
/* prototype filter of the rate converter (host code; needs no GPU).  h == NULL: only *n_h, *up, *down are written */
int32_t fw_resample_filter(int32_t rate_in, int32_t rate_out, int32_t taps_per_phase, double beta,
                           double* h, int64_t* n_h, int32_t* up, int32_t* down);
/* x[n] float32 at rate_in -> out[n_out] float32 at rate_out on HIP device `device_index`;
 * n_out must equal ceil(n * up / down); quantize_s16 != 0: the reference's s16 step (audio.py:62-66) fused:
 * clip(rint(y * 32768), -32768, 32767) / 32768.  rate_in == rate_out copies (and quantises when asked to); n == 0
 * writes nothing.  The recording passes through the device in blocks of FWAMD_RESAMPLE_BLOCK outputs (environment, read
 * per call; default 2^20), so device memory does not grow with n.  FW_ENODEV without that device: no host fallback. */
int32_t fw_resample_dev(int32_t device_index, const float* x, int64_t n, int32_t rate_in, int32_t rate_out,
                        int32_t taps_per_phase, double beta, int32_t quantize_s16, float* out, int64_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* FWAMD_H */
