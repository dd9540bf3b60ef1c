/*
 * fwamd_test.h — test and measurement hooks of libfwamd.so.  NOT part of the drop-in boundary (include/fwamd.h):
 * thin wrappers over single kernels on host buffers, so that tests/ can parity-test each kernel in isolation and
 * profiles/ can time one kernel outside the pipeline.  Nothing in faster_whisper_amd/ (the product) calls them.
 * All of them are defined in csrc/hooks.hip (fw_bench_resample: csrc/resample.hip); file names in the comments below are
 * those of the PRODUCT code a hook launches.
 */
#ifndef FWAMD_TEST_H
#define FWAMD_TEST_H

#include "fwamd.h"

#ifdef __cplusplus
extern "C" {
#endif

int32_t fw_test_gemm(fw_model* m, const float* A, const float* W, const float* bias, const float* residual,
                     int32_t M, int32_t N, int32_t K, int32_t act_gelu, int32_t use_int8, float* out);
/* one decoder linear exactly as a decode step runs it (fragment-major operands, LayerNorm folded when ln_g/ln_b are
 * given, GELU when act = 1, residual added last): x [R][K], W [N][K], bias [N] | NULL, res [R][N] | NULL ->
 * out [R][N] (row-major result) and out_from_frag [R][N] (the fragment-major copy the next linear reads, un-permuted
 * on the host).  form = 0: what a decode step launches for this row count; 1: the int8_float16 form (needs an
 * int8_float16 model; ln must be NULL); 5: the register-streaming (skinny) kernel whatever the row count, 6 / 7: that
 * kernel with one tile / 2 x 2 tiles per workgroup; 10 + cfg: the GEMM-shaped kernel of merged runs
 * (dec_gemm_big_kernel) with workgroup shape cfg, whatever the row count; any other form is refused.  0, 5, 6, 7, 10..
 * return the same bits. */
int32_t fw_test_dec_linear(fw_model* m, const float* x, const float* W, const float* bias, const float* ln_g,
                           const float* ln_b, const float* res, int32_t R, int32_t N, int32_t K, int32_t act,
                           int32_t form, float* out, float* out_from_frag);
/* the vocabulary projection of a decode step: x [R][d] raw residual rows -> float32 logits [R][n_vocab] (final
 * LayerNorm folded in fp16 mode, applied by the row quantiser in int8_float16 mode), with the model's own weights */
int32_t fw_test_dec_logits(fw_model* m, const float* x, int32_t R, float* out);
/* one launch of the logits-rules kernel (suppress lists, repetition penalty, no-repeat n-gram, timestamp rules,
 * log-softmax, top-2K candidates of cum + logp, or the Gumbel arg-max when opts selects sampling) on caller-provided
 * logits [R][n_vocab] and row state: hist [R][n] = the n tokens generated so far on each row, cum [R].  Outputs
 * cand_val / cand_tok [R][2 * beam_size] ([R][1] when sampling).  Replaces nothing in the reference: it exposes the
 * device form of CTranslate2's logits processors to tests/test_gpu_logits_rules.py. */
int32_t fw_test_logits_rules(fw_model* m, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                             const float* cum, const fw_gen_opts* opts, int32_t with_timestamps, float* cand_val,
                             int32_t* cand_tok);
/* fw_test_logits_rules plus cand_lp [R][2 * beam_size] ([R][1] when sampling): the log-prob the kernel recorded for each
 * candidate (cand_val = cum + cand_lp; -inf where the row had nothing left).  tests/test_gpu_token_logprobs_kernels.py. */
int32_t fw_test_logits_rules_lp(fw_model* m, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                                const float* cum, const fw_gen_opts* opts, int32_t with_timestamps, float* cand_val,
                                int32_t* cand_tok, float* cand_lp);
/* fw_test_logits_rules_lp for the rows of a MERGED sampling run: one launch of the sampling instantiation over R rows
 * whose temperature, seed and call differ per row — inv_temp [R] (1 / temperature), seed [R], row0 [R] (first row of the
 * row's call: the row draws its Gumbel noise as row r - row0[r] of that call; 0 <= row0[r] <= r: checked).  opts gives the
 * rules and must select sampling (beam_size 1, sampling_topk 0); its sampling_temperature and seed are not read.
 * Outputs [R][1]: the drawn token, cum + its log-prob, its log-prob.  tests/test_gpu_sampling_runs.py. */
int32_t fw_test_logits_rules_smp_tab(fw_model* m, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                                     const float* cum, const fw_gen_opts* opts, int32_t with_timestamps,
                                     const float* inv_temp, const uint64_t* seed, const int32_t* row0, float* cand_val,
                                     int32_t* cand_tok, float* cand_lp);
/* fw_test_logits_rules_lp with the state of the launch exposed (tests/test_gpu_logits_rules.py):
 *   in/out  logits [R][n_vocab]: uploaded, and downloaded WHOLE after the launch (the sparse rules edit the row in place)
 *   in      done [R / beam_size] (0 / 1: the rows of a finished chunk are skipped) | NULL: every chunk is live
 *   in      inv_temp / seed / row0 [R]: the sampling table of fw_test_logits_rules_smp_tab (opts must then select
 *           sampling) | all three NULL: sampling rows draw with opts' own temperature and seed
 *   in/out  cand_val / cand_tok / cand_lp [R][32], the kernel's own stride: the device buffers start as the caller's
 *           values and are returned whole, so slots the launch did not write keep what the caller put there
 * Checked before anything is allocated or launched (FW_EINVAL, outputs untouched): R % beam_size == 0, every hist id in
 * [0, n_vocab) — the repetition penalty and the n-gram rule index the row with them; the three older hooks check this
 * too —, every done entry 0 or 1. */
int32_t fw_test_logits_rules_ex(fw_model* m, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                const fw_gen_opts* opts, int32_t with_timestamps, const int32_t* done,
                                const float* inv_temp, const uint64_t* seed, const int32_t* row0, float* cand_val,
                                int32_t* cand_tok, float* cand_lp);
/* fw_test_logits_rules_ex plus alternatives (tests/test_gpu_alternatives_kernels.py): the ALT instantiations of the rules
 * kernel, which also write the first n_alt rounds of every live row's extraction.
 *   in      n_alt in [1, FW_MAX_ALTERNATIVES] (checked: FW_EINVAL, outputs untouched)
 *   in/out  alt_tok / alt_lp [R][n_alt]: the device slab of step n starts as the caller's values, so the rows of a chunk
 *           marked done keep them; a live row gets its n_alt best (log-prob descending, id ascending), (0, -inf) once
 *           nothing is left.  Sampling rows: the draw in cand_*, the plain top n_alt here. */
int32_t fw_test_logits_rules_alt(fw_model* m, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                 const fw_gen_opts* opts, int32_t with_timestamps, const int32_t* done,
                                 const float* inv_temp, const uint64_t* seed, const int32_t* row0, float* cand_val,
                                 int32_t* cand_tok, float* cand_lp, int32_t n_alt, int32_t* alt_tok, float* alt_lp);
/* fw_test_logits_rules_alt plus per-row truncation limits (tests/test_gpu_sampling_trunc_kernel.py): ONE launch of the
 * TRUNC instantiation of the rules kernel, whatever the rows' limits are.
 *   in      top_k / top_p [R]: the launch's second per-row table, beside inv_temp / seed / row0; top_k >= 0, top_p in
 *           (0, 1] (checked: FW_EINVAL); a row with (0, 1.0) must get the bits of the plain sampling kernel
 *   in      n_alt in [0, FW_MAX_ALTERNATIVES]; with n_alt == 0 alt_tok / alt_lp are NULL
 * opts must select sampling (beam_size 1, sampling_topk 0).  Everything else as fw_test_logits_rules_alt. */
int32_t fw_test_logits_rules_trunc(fw_model* m, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                   const fw_gen_opts* opts, int32_t with_timestamps, const int32_t* done,
                                   const float* inv_temp, const uint64_t* seed, const int32_t* row0, const int32_t* top_k,
                                   const float* top_p, float* cand_val, int32_t* cand_tok, float* cand_lp, int32_t n_alt,
                                   int32_t* alt_tok, float* alt_lp);
/* ONE launch of the scoring kernel (dec_score_kernel, what fw_score launches per position block) on caller-provided rows
 * (tests/test_gpu_score_kernel.py):
 *   in/out  logits [rows][n_vocab] float32: uploaded, and downloaded WHOLE after the launch (the kernel must not write it)
 *   in      targets [rows]: the id scored on each row; < 0: the row has no target and nothing is written for it
 *   in      hist, hist_offsets [rows + 1]: row r's history is hist[hist_offsets[r] .. hist_offsets[r + 1]), fewer than
 *           n_text_ctx ids (read only with rules; hist may be NULL when every history is empty)
 *   in      opts | NULL: NULL scores the raw distribution; otherwise the decoding rules of a greedy row with that history
 *           (repetition_penalty, no_repeat_ngram_size, suppress_blank, suppress_tokens, max_initial_timestamp_index;
 *           with_timestamps switches the timestamp rules; every other field is ignored)
 *   in/out  out_lp / out_best_id / out_best_lp [rows]: the device buffers start as the caller's values
 * Checked before anything is allocated or launched (FW_EINVAL): targets below n_vocab, every hist id in [0, n_vocab),
 * offsets that do not decrease, histories shorter than n_text_ctx. */
int32_t fw_test_score_rows(fw_model* m, float* logits, int32_t rows, const int32_t* targets, const int32_t* hist,
                           const int32_t* hist_offsets, const fw_gen_opts* opts, int32_t with_timestamps, float* out_lp,
                           int32_t* out_best_id, float* out_best_lp);
/* out[0] = step graphs (one hipGraph per distinct decode-step geometry, decoder.hip) the model's decode group has
 * captured and instantiated since the model was created, summed over its lanes */
int32_t fw_test_graph_captures(const fw_model* m, int64_t* out);
/* The three hooks of the decode-state kernels (tests/test_gpu_decode_state.py).  Geometry comes from the arguments, not
 * from the model.  Every quantity a kernel uses as an index or extent is checked BEFORE anything is allocated or
 * launched; a violation returns FW_EINVAL (a wrong test gets an error code, never a device fault).
 *
 * fw_test_dec_beam_update: one launch of the beam update (dec_kernels.hip K19/K20: launch_beam_update) for B chunks of K
 * beams (R = B * K rows) at decode step `step` of a text context of NT positions and a vocabulary of V tokens.
 *   in      cand_val / cand_tok [R][2 K] (each row sorted by value, descending, -inf at the tail: what the logits-rules
 *           kernel leaves; the hook places them at the kernel's stride of 32 per row), hist [R][step], kvidx
 *           [R][P - 1 + step], cum [R]
 *   in/out  done [B], n_done [1], n_fin [B], fin_tok [B][FIN_CAP = 48][NT], fin_len / fin_score / fin_cum [B][48]: uploaded
 *           and downloaded WHOLE
 *   out     hist2 [2][R][NT], kvidx2 [2][R][NT] (bytes), cum2 [2][R], cur_tok [R]: both parity halves whole.  The hook put
 *           hist / kvidx / cum into half step & 1 and filled everything else (the rest of that half, the other half,
 *           cur_tok) with sentinel_i (its low byte in kvidx2) / sentinel_f (cum2) before the launch.
 * Checked: 1 <= K <= 16, 1 <= B <= 4096, 1 <= NT <= 4096, P >= 1, 0 <= step < NT, P - 1 + step < NT, 0 <= eot < V,
 * max_fin >= 1, budget >= 1, every cand_tok in [0, V), every kvidx byte < K, 0 <= n_fin[c] <= 48. */
int32_t fw_test_dec_beam_update(fw_model* m, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                const int32_t* cand_tok, const int32_t* hist, const uint8_t* kvidx, const float* cum,
                                int32_t sentinel_i, float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin,
                                int32_t* fin_tok, int32_t* fin_len, float* fin_score, float* fin_cum, int32_t* hist2,
                                uint8_t* kvidx2, float* cum2, int32_t* cur_tok);
/* fw_test_dec_beam_update plus the per-token log-prob state (tests/test_gpu_token_logprobs_kernels.py):
 *   in      cand_lp [R][2 K] beside cand_val / cand_tok, lphist [R][step] beside hist
 *   in/out  fin_lp [B][48][NT + 1]: a finished hypothesis' token log-probs, at [NT] that of its <eot> (0: cut at the
 *           budget); uploaded and downloaded whole
 *   out     lphist2 [2][R][NT]: both parity halves whole; lphist went into half step & 1, the rest holds sentinel_f */
int32_t fw_test_dec_beam_update_lp(fw_model* m, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                   int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                   const int32_t* cand_tok, const float* cand_lp, const int32_t* hist,
                                   const float* lphist, const uint8_t* kvidx, const float* cum, int32_t sentinel_i,
                                   float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin, int32_t* fin_tok,
                                   int32_t* fin_len, float* fin_score, float* fin_cum, float* fin_lp, int32_t* hist2,
                                   float* lphist2, uint8_t* kvidx2, float* cum2, int32_t* cur_tok);
/* fw_test_dec_beam_update_lp plus the path of a finished hypothesis and ragged launches
 * (tests/test_gpu_alternatives_kernels.py):
 *   in      ptab [B] | NULL: chunk c has a prompt of ptab[c] tokens (the RAGGED instantiation).  P must then be the
 *           shortest, the run reaches P + budget positions, kvidx is [R][max(ptab) - 1 + step] and the rows of chunk c use
 *           the first ptab[c] - 1 + step bytes of theirs.  Checked: P <= ptab[c], ptab[c] - 1 + step < min(NT, P + budget)
 *   in/out  fin_path [B][48][NT + 1] bytes | NULL (the kernel gets a null pointer: fw_test_dec_beam_update_lp bit for
 *           bit): for a hypothesis recorded at this step, byte q < step = its source row's kvidx byte at ptab[c] - 1 + q,
 *           byte step = the source row's beam index; uploaded and downloaded whole */
int32_t fw_test_dec_beam_update_alt(fw_model* m, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                    int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                    const int32_t* cand_tok, const float* cand_lp, const int32_t* hist,
                                    const float* lphist, const uint8_t* kvidx, const float* cum, int32_t sentinel_i,
                                    float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin, int32_t* fin_tok,
                                    int32_t* fin_len, float* fin_score, float* fin_cum, float* fin_lp, int32_t* hist2,
                                    float* lphist2, uint8_t* kvidx2, float* cum2, int32_t* cur_tok, const int32_t* ptab,
                                    uint8_t* fin_path);
/* ONE launch of the alternatives gather (what a decode run launches once after its last step):
 *   in      alt_tok / alt_lp [steps][R][n_alt] (step-major, as the rules kernel writes them), fin_path [R / K][48][NT + 1]
 *   in      n_hyp hypotheses: decode chunk, finished slot, length, and the step whose row produced the closing <eot>
 *           (-1: cut at the budget, no closing step)
 *   in/out  out_tok / out_lp [n_hyp][T + 1][n_alt]: entry t < len = alt_*[t][chunk * K + path[t]], entry T = those of
 *           the closing step; entries in [len, T), and entry T without a closing step, are (-1, 0)
 * Checked: 1 <= n_alt <= FW_MAX_ALTERNATIVES, 1 <= K <= 16, R % K == 0, R <= 4096, 1 <= NT <= 4096, 1 <= steps <= NT + 1,
 * 0 <= T <= NT, chunk < R / K, slot < 48, 0 <= len <= min(T, steps), -1 <= end < steps, every path byte read < K. */
int32_t fw_test_alt_gather(fw_model* m, const int32_t* alt_tok, const float* alt_lp, int32_t steps, int32_t R, int32_t K,
                           int32_t NT, int32_t n_alt, const uint8_t* fin_path, int32_t n_hyp, const int32_t* hyp_chunk,
                           const int32_t* hyp_fin, const int32_t* hyp_len, const int32_t* hyp_end, int32_t T,
                           int32_t* out_tok, float* out_lp);
/* ONE launch of dec_boost_kernel (phrase boosting, include/fwamd.h) in either row form on caller-provided rows: logits
 * [rows][n_vocab] IN / OUT, returned whole; row r's generated history is hist[hist_offsets[r] .. hist_offsets[r + 1])
 * (hist_offsets[0] == 0; hist may be NULL when every history is empty).
 *   form 0, the decode step: every row has the SAME n (uniform offsets: checked), the histories are laid out as the
 *           parity half of hist2 that step n selects and the device step counter holds n; rows % K == 0, 1 <= K <= 16;
 *           done [rows / K] (0 / 1: checked) | NULL: the rows of a done chunk are skipped;
 *   form 1, scoring: one ScoreRow per row, ragged histories; K must be 1; done [rows] | NULL: a row with done[r] != 0 has
 *           no target (target < 0) and is skipped.
 * Checked before anything is allocated or launched: the pointers, rows >= 1, form, K, every n < n_text_ctx, every history
 * id in [0, n_vocab), the done values, and that the list was built for the model's n_vocab. */
int32_t fw_test_boost_rows(fw_model* m, float* logits, int32_t rows, const int32_t* hist, const int32_t* hist_offsets,
                           int32_t K, const int32_t* done, int32_t form, const fw_boost* boost);
/* host-only (no device, no model needed): the same table walked in plain C++ over logits [rows][n_vocab of the list]
 * IN / OUT with ragged histories as above — what fw_boost_create compiled, testable without a GPU */
int32_t fw_test_boost_rows_host(float* logits, int32_t rows, const int32_t* hist, const int32_t* hist_offsets,
                                const fw_boost* boost);
/* ONE launch of dec_constrain_kernel (constrained decoding, include/fwamd.h) in either row form on caller-provided rows,
 * with the rows, histories, K, done and form of fw_test_boost_rows above.  The model gives the device, the stream and the
 * text context only: the vocabulary geometry is the caller's — logits [rows][n_vocab] IN / OUT, returned whole, <eot> =
 * tok_eot, timestamp ids from tok_ts_begin, with_timestamps 1 (the timestamp rules are on: those ids keep their bits) / 0 —
 * so a test chooses n_vocab mod 4 and with it the alignment of every row.  Checked before anything is allocated or
 * launched: what fw_test_boost_rows checks, 0 <= tok_eot < tok_ts_begin <= n_vocab <= 57344, with_timestamps 0 / 1, and
 * that the list was built for n_vocab.  The ids of the list are NOT checked against tok_eot (fw_generate_constrain's
 * check): an id >= tok_ts_begin in a phrase allows nothing. */
int32_t fw_test_constrain_rows(fw_model* m, float* logits, int32_t rows, int32_t n_vocab, int32_t tok_eot,
                               int32_t tok_ts_begin, int32_t with_timestamps, const int32_t* hist, const int32_t* hist_offsets,
                               int32_t K, const int32_t* done, int32_t form, const fw_constraint* constraint);
/* host-only (no device, no model needed): the same table walked in plain C++, ragged histories of any length */
int32_t fw_test_constrain_rows_host(float* logits, int32_t rows, int32_t n_vocab, int32_t tok_eot, int32_t tok_ts_begin,
                                    int32_t with_timestamps, const int32_t* hist, const int32_t* hist_offsets,
                                    const fw_constraint* constraint);
/* host-only: the compiled table of a list (what the merge rule compares).  *out_words = its size in 32-bit words; out
 * (NULL with cap == 0) receives the first min(cap, size) words */
int32_t fw_test_constraint_table(const fw_constraint* constraint, int32_t* out, int32_t cap, int32_t* out_words);
/* one launch of the token + position embedding (K12: launch_embed): tok [rows] (in [0, V): checked), emb [V][d], pos_emb
 * [NT][d] (rounded to fp16 by the hook) -> x [rows][d] and x_frag [ceil(rows / 16) * 16][d], the fragment-major copy
 * un-permuted on the host; its device buffer starts as `sentinel`, so the padding rows of the last tile stay visible.
 * Position of row r: blk_n > 0 (<= 16, rows % blk_n == 0, pos_fixed >= 0, pos_fixed + blk_n <= NT): pos_fixed + r % blk_n;
 * else pos_fixed >= 0 (< NT): pos_fixed; else the step-counter route, P - 1 + step (P >= 1, 0 <= step, < NT).
 * d % 32 == 0. */
int32_t fw_test_dec_embed(fw_model* m, const int32_t* tok, int32_t rows, const float* emb, int32_t V,
                          const float* pos_emb, int32_t NT, int32_t d, int32_t pos_fixed, int32_t P, int32_t step,
                          int32_t blk_n, float sentinel, float* x, float* x_frag);
/* the device part of align's post-processing, align_stats_kernel then align_filter_kernel launched as fw_align does:
 * probs [B][n_sel][n_tok_cap][T], n_tok [B] (1 .. n_tok_cap), nfr [B] (1 .. T), width odd and <= 15, n_sel >= 1 ->
 * mat [B][n_tok_cap][T] IN / OUT (the device buffer starts as the caller's values; only tok < n_tok[b], t < nfr[b] are
 * written).  A frame with zero variance over the tokens gives inf * 0 here and in the oracle alike: not pinned. */
int32_t fw_test_align_post(fw_model* m, const float* probs, int32_t B, int32_t n_sel, int32_t n_tok_cap, int32_t T,
                           const int32_t* n_tok, const int32_t* nfr, int32_t width, float* mat);
/* measurement hook (profiles/gemm_bench.py): average milliseconds of one launch of the "many rows" GEMM
 * C[batch][M][N] = A[batch][M][K] W[N][K]^T on device-resident pseudo-random operands (fp16, or int8 on an
 * int8_float16 model); lda = K + a_pad, ldw = K + w_pad elements; trans: the transposed-output form */
int32_t fw_bench_gemm(fw_model* m, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t a_pad, int32_t w_pad,
                      int32_t trans, int32_t iters, float* ms_out);
/* micro-benchmark of the decoder linear kernel (dec_gemm_frag_kernel) for a tile-shape `variant` (dec_kernels.hip:
 * launch_dec_gemm_frag_variant; 0 / 1 = the product's skinny kernel, 10 + cfg = the GEMM-shaped kernel of merged runs) over a rotating weight set larger than the caches:
 * mean microseconds per launch of a [R] x [N][K] linear (lnf = LayerNorm-folded form). */
int32_t fw_bench_dec_linear(fw_model* m, int32_t R, int32_t N, int32_t K, int32_t lnf, int32_t variant, int32_t iters,
                            float* us_out);
/* fw_bench_gemm with the epilogue the product runs for the shape (profiles/gemm_bench.py --epilogue; float16 models):
 * bias != 0: a bias vector; act = 1: GELU; res = 1: a residual [batch][M][N] read from buffers larger than the caches,
 * rotated launch by launch; res = 2: one [M][N] block shared by the chunks (conv2's positional embedding); lda: row
 * stride of A in elements (0: K; conv2 reads overlapping rows, lda = 2 d, K = 3 d); n_layers > 1: the layered
 * head-major cross-attention K (trans = 0) / V^T (trans = 1) projection, N = d_model per layer, no residual */
int32_t fw_bench_gemm_epi(fw_model* m, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t lda, int32_t trans,
                          int32_t bias, int32_t act, int32_t res, int32_t n_layers, int32_t iters, float* ms_out);
/* fw_bench_dec_linear with the epilogue a decode step runs (profiles/dec_linear_bench.py --epilogue): act = 1: GELU;
 * res = 1: the residual added in place (res == out, rows rotated over buffers larger than the caches); outs bit 0: the
 * row-major copy is written, bit 1: the fragment-major copy.  variant 0: what a decode step launches for this row
 * count, 5: the register-streaming kernel, 10 + cfg: the GEMM-shaped kernel of merged runs */
int32_t fw_bench_dec_linear_epi(fw_model* m, int32_t R, int32_t N, int32_t K, int32_t lnf, int32_t variant, int32_t act,
                                int32_t res, int32_t outs, int32_t iters, float* us_out);
int32_t fw_test_layernorm(fw_model* m, const float* x, const float* g, const float* b,
                          int32_t rows, int32_t d, float* out);
/* fw_test_layernorm with the output layout as an argument: frag = 1 is the MFMA-fragment-major form the decoder linears
 * read (rowops.hip; d % 32 == 0), un-permuted on the host into out [rows][d]; frag = 0 is fw_test_layernorm */
int32_t fw_test_layernorm_frag(fw_model* m, const float* x, const float* g, const float* b, int32_t rows, int32_t d,
                               int32_t frag, float* out);
/* one launch of the row quantiser (rowops.hip: launch_quant_rows): x [rows][ldx] (the first d of every ldx elements are
 * a row; ldx % 8 == 0, ldx >= d), LayerNorm in front when ln_g / ln_b are given -> int8 codes xq [rows][d] and
 * de-quantisation scales scale [rows].  frag = 1: the int8 fragment-major destination, un-permuted on the host.
 * d % 64 == 0; d <= 1536 with LayerNorm, <= 5120 without (the kernel's limits). */
int32_t fw_test_quant_rows(fw_model* m, const float* x, int32_t rows, int32_t d, int64_t ldx, const float* ln_g,
                           const float* ln_b, int32_t frag, int8_t* xq, float* scale);
/* one launch of the encoder GEMM in any form the product launches, through the product's entry point (engine.hip:
 * run_linear; use_int8: quantise_rows into the model's quantisation workspace first — FW_EINVAL when batch * M rows of K
 * do not fit it).  The caller describes the device buffers as they lie in memory (all counts in elements):
 *   A    a_elems values; chunk z, row r starts at z * a_bstride + r * lda (rows may overlap: conv2 has lda < K).
 *        use_int8: contiguous [batch * M][K] (lda = K, a_bstride = M * K: what quantise_rows takes), quantised by the
 *        product's row quantiser, through LayerNorm(ln_g, ln_b [K]) when those are given
 *   W    [n_layers][N][K], bias [n_layers][N] | NULL (use_int8: W quantised per row on the host like fw_test_gemm)
 *   res  r_elems values | NULL; chunk z, row r at z * r_bstride + r * ldr (r_bstride = 0: one block shared by all
 *        chunks); row-major output only
 *   C    c_elems values IN / OUT: the WHOLE buffer is uploaded (rounded to fp16) before the launch and downloaded after
 *        it, gaps and tail included, and nothing is un-permuted.  The launch gets C + c_off (c_off % 8 == 0); layer l,
 *        chunk z start at l * c_lstride + z * c_bstride.  Row-major: row r at r * ldc; trans = 1: Ct, column n at
 *        n * ldc; head_rows > 0 (% 32 == 0, >= M, N % 64 == 0): the fragment-major cross-attention K (trans = 0) / V^T
 *        (trans = 1) block of [N / 64][head_rows * 64] per chunk (index it with fw_test_cross_kv_frag_index)
 * Before anything is launched the furthest element the described launch reads or writes in A, res and C is computed:
 * FW_EINVAL when it lies outside a_elems / r_elems / c_elems (a wrong test gets an error code, never a device fault). */
int32_t fw_test_gemm_ex(fw_model* m, const float* A, int64_t a_elems, int64_t lda, int64_t a_bstride, const float* W,
                        const float* bias, const float* res, int64_t r_elems, int64_t ldr, int64_t r_bstride, float* C,
                        int64_t c_elems, int64_t c_off, int64_t ldc, int64_t c_bstride, int64_t c_lstride, int32_t M,
                        int32_t N, int32_t K, int32_t batch, int32_t n_layers, int32_t act, int32_t trans,
                        int32_t head_rows, int32_t use_int8, const float* ln_g, const float* ln_b);
/* host-only: idx [kvp][N] = position of (key, column) inside one chunk's fragment-major cross-attention K (vt = 0) /
 * V^T (vt = 1) block of [N / 64][kvp * 64] halves (kvp % 32 == 0, N % 64 == 0): the layout the projection GEMM writes */
int32_t fw_test_cross_kv_frag_index(int32_t vt, int32_t kvp, int32_t N, int64_t* idx);
int32_t fw_test_attention(fw_model* m, const float* q, const float* k, const float* v,
                          int32_t B, int32_t H, int32_t T, float* out);
/* decoder self-attention, one launch exactly as a decode step makes it (dec_kernels.hip: launch_self_attn; the form
 * follows knob 2): qkv [R][3 d] (d = H * 64, R = n_chunks * kmul), K / V cache kcache / vcache
 * [n_chunks * Kbeam][H][cache_ctx][64] IN / OUT (returned as the launch leaves it: the new K / V of each row written at
 * its position of its own slot), slot table kvidx [2][n_chunks * Kbeam][n_ctx] (every byte < Kbeam: checked) ->
 * out [R][d].  Position pos_fixed, or with pos_fixed < 0 the step counter route: the device step counter holds `step`,
 * pos = P - 1 + step and the slot table half step & 1 is read.  blk_n > 0 (needs kmul == blk_n, pos_fixed >= 0):
 * position blocks, row c * blk_n + j = position pos_fixed + j of chunk c's beam slot 0.  frag = 1: the fragment-major
 * output of the fp16 path, un-permuted on the host; 0: the row-major output of the int8 path (the same values). */
int32_t fw_test_dec_self_attn(fw_model* m, const float* qkv, float* kcache, float* vcache, const uint8_t* kvidx,
                              int32_t n_chunks, int32_t kmul, int32_t Kbeam, int32_t H, int32_t n_ctx, int32_t cache_ctx,
                              int32_t pos_fixed, int32_t P, int32_t step, int32_t blk_n, int32_t frag, float* out);
/* decoder cross-attention, one launch of launch_cross_attn (register cap: knob 7): q [B * kmul][d] (kmul <= 16),
 * k / v [n_enc][T][d] plain row-major, laid out by the hook in the pool's fragment-major K / V^T (kvp = T rounded up
 * to 32 keys; K's padded keys hold k_pad, V^T's zeros: the pool's contract).  Decode chunk c attends to encoder chunk
 * slot_map[c / kv_div] (slot_map [ceil(B / kv_div)], values < n_enc: checked); chunks with done[c] != 0 (done [B] or
 * NULL) are skipped.  out [B * kmul][d] IN / OUT: the device output starts as the caller's values. */
int32_t fw_test_dec_cross_attn(fw_model* m, const float* q, const float* k, const float* v, int32_t n_enc, int32_t T,
                               int32_t H, int32_t B, int32_t kmul, int32_t kv_div, const int32_t* slot_map,
                               const int32_t* done, int32_t frag, float k_pad, float* out);
/* the cross-attention probabilities of align (launch_cross_probs): q [B * blk][d] (blk = max(blk_n, 1) <= 16: row
 * b * blk + j is token tok_idx + j of chunk b), k [B][T][d] (laid out as the pool's K), heads [n_sel] (< H) ->
 * probs [B][n_sel][n_tok][T] float32 IN / OUT: only token slots tok_idx .. tok_idx + blk - 1 are written. */
int32_t fw_test_dec_cross_probs(fw_model* m, const float* q, const float* k, int32_t B, int32_t T, int32_t H,
                                const int32_t* heads, int32_t n_sel, int32_t n_tok, int32_t tok_idx, int32_t blk_n,
                                float* probs);
/* fp32 softmax picks of a decode step on float32 logits [rows * row_mul][V] (row b reads logits row b * row_mul):
 * nospeech = 1: dec_nospeech_kernel, out[b] = softmax(row)[target[0]] (target[0] < V: checked); 0:
 * dec_token_prob_kernel, out[b] = softmax(row)[target[b]], 0 for a target outside [0, V). */
int32_t fw_test_dec_softmax_pick(fw_model* m, const float* logits, int32_t rows, int32_t V, int32_t row_mul,
                                 const int32_t* target, int32_t nospeech, float* out);
/* measurement hook (profiles/attn_bench.py): mean milliseconds of one launch of the encoder self-attention kernel for
 * B chunks x H heads x T positions on device-resident pseudo-random operands; variant = the workgroup mapping
 * (0: XCD-aware, the product's; 1: query tile fastest over all XCDs, round 3's) */
int32_t fw_bench_attention(fw_model* m, int32_t B, int32_t H, int32_t T, int32_t variant, int32_t iters, float* ms_out);
/* measurement hook (profiles/resample_bench.py): mean milliseconds of the rate-conversion kernel of fw_resample_dev over
 * the whole of x[n] (uploaded once, every output in one launch, `iters` launches between two HIP events after a warm-up) */
int32_t fw_bench_resample(int32_t device_index, const float* x, int64_t n, int32_t rate_in, int32_t rate_out,
                          int32_t taps_per_phase, double beta, int32_t quantize_s16, int32_t iters, float* ms_out);

/* rows from which a decode run's per-layer linears take the GEMM-shaped kernel (dec_kernels.hip: dec_linear_plan's table);
 * bench.py prices the decoder linears against the MFMA roof from this row count on, against HBM below */
int32_t fw_dec_big_min_rows(void);
/* the same per linear: role 0 qkv, 1 d x d (out / cross-q / cross-out), 2 ffn1, 3 ffn2 (< 0: the lowest of the four);
 * compute_type 0 float16, 1 int8_float16 (one row count for every linear).  Each linear switches at its own measured
 * crossover, so a run between the lowest and the highest has some linears on either kernel: bench.py prices per role */
int32_t fw_dec_big_min_rows_of(int32_t role, int32_t compute_type);
/* process-wide measurement knob for A/B runs inside one process.  id 1: encoder GEMM tile order (1 = blocked, the
 * product's; 0 = n fastest across the whole width, rounds 1-3).  id 2: decoder self-attention form (0 = by launch size,
 * the product's; 1 = the first form of rounds 1-4; 2 = latency form; 3 = throughput form — all four return the same bits).  id 4 (3 was the weight prefetch of
 * solo runs, measured slower twice and removed: profiles/r05_ab_wprefetch_*.jsonl): position blocks for the prompt forward and align (1, the default:
 * up to 16 positions per decoder pass; 0: one position per pass, rounds 1-4 — the same bits).  id 5: the plain transposed
 * GEMM epilogue, i.e. the encoder's V^T (1, the default: staged through LDS, whole row segments of Ct; 0: direct 8-byte stores,
 * rounds 1-4 — the same bits).  id 6: the cross-attention K / V^T projections (1, the default: all decoder layers in two
 * launches of the encoder GEMM; 0: two launches per layer, rounds 1-4 — the same bits).  id 7: register cap of the decoder
 * cross-attention kernel (0, the default: none, 110 registers; 1: 96; 2: 80 — the same bits; profiles/r06_ab_cross_regs.jsonl) */
int32_t fw_test_knob(int32_t id, int32_t value);
/* host-only (no device needed): chunks an IDLE two-lane decode group wants queued before it leads a run — its even share of
 * the work it knows of (`queued` chunks in `n_queued` requests + one request of that average size per worker inside an encode
 * call) over the runs that work needs (>= 2; `want` = chunks one run takes), at least one batch.  The rule the leader of a
 * run applies when no run is in progress (fw_model_set_merge_wait, include/fwamd.h). */
int64_t fw_test_idle_lead_chunks(int64_t queued, int32_t n_queued, int32_t encoding, int64_t want, int32_t max_batch);
/* host-only (no device needed): what a decode lane of `lane_chunks` chunks x `max_beam` rows, with a self-attention cache of
 * `self_cap` row-positions, holds of runs led by a call of `B` chunks (beam_size, or num_hypotheses sampled rows per chunk
 * when `sampling`; ctx = cache positions per row at the call's max_length).  Returns 1 when the call alone fits the lane
 * (fw_generate refuses it otherwise), 0 when not; *rows_per_chunk = decoder rows per encoder chunk; *want = chunks the
 * leader of the run waits for (0: it does not wait: sampling); *run_cap = chunks the run is filled to. */
int32_t fw_test_run_capacity(int32_t lane_chunks, int32_t max_batch, int32_t max_beam, int64_t self_cap, int32_t B,
                             int32_t sampling, int32_t beam_size, int32_t num_hypotheses, int32_t ctx,
                             int64_t* rows_per_chunk, int64_t* want, int64_t* run_cap);
/* host-only (no device needed): the kernel form a decoder linear of R rows and [N][K] weights takes (dec_kernels.hip:
 * dec_linear_plan, the one place that decides it); ldo / ldr: row strides of the output and the residual in elements
 * (ldr = 0: no residual); compute_type 0 float16, 1 int8_float16; form as in fw_test_dec_linear (0, 5, 6, 7, 10 + cfg).
 * out[0] family (0 refused, 1 the skinny kernel — the int8 kernel counts as skinny —, 2 the GEMM-shaped kernel),
 * out[1] cfg of the GEMM-shaped kernel (-1 otherwise), out[2] / out[3] / out[4] skinny: 16 x 16 row tiles / column tiles
 * per workgroup and k-steps of loads in flight per wave (0 otherwise), out[5] waves K is split over (4 | 8) */
int32_t fw_test_dec_linear_plan(int32_t R, int32_t N, int32_t K, int32_t ldo, int32_t ldr, int32_t compute_type,
                                int32_t form, int32_t out[6]);
/* host-only (no device needed): what the encoder GEMM's launcher does for a launch of C[batch][M][N] = A[batch][M][K]
 * W[N][K]^T (gemm.hip: gemm_plan, the one place that decides it) under the current knobs 1 and 5.  Strides in elements;
 * int8 0: fp16 operands, 1: int8 codes with both scales, 2: int8 codes without the weight scale; has_res: a residual.
 * out[0] instantiation (-1: the shape is refused and nothing would be launched; else trans + 2 * int8, layered 4 + trans),
 * out[1] m tiles of a chunk, out[2] n tiles of all layers, out[3] n tiles of one layer, out[4] m panels of the batch,
 * out[5] / out[6] the tile-order block in n tiles / m panels (0 / 0: n fastest across the width), out[7] vt_stage,
 * out[8] workgroups */
int32_t fw_test_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t batch, int64_t lda, int64_t ldw, int64_t a_bstride,
                          int64_t ldc, int64_t c_bstride, int32_t trans, int32_t int8, int32_t head_rows, int32_t n_layers,
                          int32_t has_res, int32_t out[9]);
/* host-only (no device needed): the form (1 first, 2 latency, 3 throughput) the decode self-attention takes for `chunks`
 * chunks of kmul rows and H heads under knob 2's value `knob`; n_ctx / cache_ctx / d / R_total: the cache geometry as in
 * fw_test_dec_self_attn (R_total = cache slots per layer) */
int32_t fw_test_self_attn_form(int32_t n_ctx, int32_t cache_ctx, int32_t d, int32_t R_total, int32_t kmul, int32_t H,
                               int32_t chunks, int32_t knob);
/* host-only (no device needed): the checks model creation makes of a weight blob before it binds it, on a HOST copy of
 * `bytes` bytes — header (magic, version, size, config, compute type, layout generation), then for every tensor the
 * weight list expects for that config and compute type: present, dtype, ndim / dims (the stored extent of fragment-major
 * tensors), nbytes = dims x element size, offset % 256 == 0, offset + nbytes <= total_bytes.  FW_OK, or FW_EINVAL with
 * the tensor's name in fw_last_error. */
int32_t fw_test_blob_check(const void* blob_host, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* FWAMD_TEST_H */
