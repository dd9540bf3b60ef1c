// Launch API of the decoder-step kernels (dec_kernels.hip; the kernels that hold one vocabulary row: dec_vocab.hip).
#pragma once
#include <vector>

#include "../../include/fwamd.h"
#include "common.h"

namespace fwd {

constexpr int FIN_CAP = 48;  // finished hypotheses kept per chunk (>= round(K*patience) + K)
// 64-bit words of the suppress mask (one bit per token id, zero-padded past the vocabulary): 56 * 1024 ids, what a
// workgroup of the rules kernel holds in registers
#define LP_SUP_WORDS 896

// Per-generate constants handed to the kernels by value.
struct GenDev {
  int B, K, R;             // chunks, beams per chunk, rows = B*K
  int P;                   // prompt length (all prompts of a call have the same length)
  int budget;              // max new tokens
  int max_fin;             // round(K * patience)
  int V, n_text_ctx;
  int with_ts, suppress_blank, min_new, mits, ngram;
  float rep_pen, lp_pow;
  int eot, no_ts, ts_begin;
  int n_sup_begin, sup_begin[8];
  int sample;              // 1: draw the next token from softmax(logp / T) instead of arg-max / beam
  // (sampling runs read temperature and seed per row from a SmpRow table: decode runs set these three to 1, 0, 0, so
  //  that sampling runs of one size share a step graph whatever their calls' seeds and temperatures)
  float inv_temp;
  unsigned seed_lo, seed_hi;
  int kv_div;              // decode chunks per encoder chunk (sampling: num_hypotheses), 1 otherwise
  int ctx, cache_rows;     // self-attention cache geometry of this run: positions per slot, slots per layer
  // RAGGED run (calls of different prompt lengths in one run): the step kernels take each chunk's prompt length from a
  // device table instead of P, `reach` = min(max_length, n_text_ctx) is where every chunk's budget ends; P is then the
  // shortest prompt and budget the longest budget.  0 / 0 in a uniform run: a cached step graph captured the table
  // pointer (or null) by value, so the two kinds never share a graph.
  int ragged, reach;
  // ALTERNATIVES (fw_generate_alt): the rules kernel also records the row's n_alt most likely ids per step (the largest
  // n_alt of the run's calls, <= FW_MAX_ALTERNATIVES).  0 in every run that records none: the key and the kernels of today.
  int n_alt;
  // BOOST (fw_generate_boost): 1 when the step launches dec_boost_kernel in front of the rules kernel.  0 in every run
  // without a list: the key and the graphs of today.  The table's sizes travel in the table's header, not here.
  int boost;
  // TRUNC (fw_generate_trunc): 1 when some call of a sampling run limits its draw (top_k > 0 or top_p < 1): the step then
  // launches the TRUNC instantiations of the rules kernel, which read a TruncRow per row.  0 in every other run: the key,
  // the kernels and the graphs of today.
  int trunc;
  // CONSTRAIN (fw_generate_constrain): 1 when the step launches dec_constrain_kernel between the boost and the rules
  // kernel.  0 in every run without a list: the key, the kernels and the graphs of today.  The table's sizes travel in the
  // table's header, not here.
  int constrain;
};

// GenDev::mits from the caller's max_initial_timestamp_index (unbounded there: CTranslate2 takes a size_t).  The rules
// kernel forbids ids from ts_begin + mits + 1 on at the first step, in int arithmetic: a limit at or past the number of
// timestamp ids forbids nothing, and so does a negative one — both become -1, "no limit", which also gives equivalent
// values one step-graph key.  fill_rule_fields (below) fills mits through this.
static inline int initial_timestamp_limit(long long max_initial_timestamp_index, int n_vocab, int ts_begin) {
  const long long n_ts = (long long)n_vocab - ts_begin;
  return (max_initial_timestamp_index < 0 || max_initial_timestamp_index >= n_ts) ? -1 : (int)max_initial_timestamp_index;
}

// THE place that fills the rule fields of GenDev (what the rules kernel and the scoring kernel read of the caller's
// options and of the model's token ids).  o == null: no rule at all, the raw distribution (the scoring paths).
static inline void fill_rule_fields(GenDev& gp, const fw_config& c, const fw_gen_opts* o, int with_ts) {
  gp.with_ts = (o && with_ts) ? 1 : 0;
  gp.suppress_blank = (o && o->suppress_blank) ? 1 : 0;
  gp.min_new = o ? o->min_new_tokens : 0;
  gp.mits = o ? initial_timestamp_limit(o->max_initial_timestamp_index, c.n_vocab, c.tok_timestamp_begin) : -1;
  gp.ngram = o ? o->no_repeat_ngram_size : 0;
  gp.rep_pen = o ? o->repetition_penalty : 1.0f;
  gp.eot = c.tok_eot; gp.no_ts = c.tok_no_timestamps; gp.ts_begin = c.tok_timestamp_begin;
  gp.n_sup_begin = o ? c.n_suppress_begin : 0;
  for (int i = 0; i < gp.n_sup_begin; ++i) gp.sup_begin[i] = c.suppress_begin[i];
}

// The suppress list as the kernels read it: one bit per token id, LP_SUP_WORDS 64-bit words; ids outside the vocabulary
// are dropped.
static inline std::vector<unsigned long long> suppress_mask(const int32_t* tokens, int n_tokens, int n_vocab) {
  std::vector<unsigned long long> mask(LP_SUP_WORDS, 0ull);
  for (int i = 0; i < n_tokens; ++i) {
    const int t = tokens[i];
    if (t >= 0 && t < n_vocab) mask[t >> 6] |= 1ull << (t & 63);
  }
  return mask;
}

// Sampling runs: one entry per decode row.  The calls of a run keep their own temperature and seed, and a row draws its
// noise as row `r - row0` of its call: what it is in a run of that call alone.
struct SmpRow {
  float inv_temp;
  unsigned seed_lo, seed_hi;
  int row0;                // first row of the entry's call inside the run
};
static_assert(sizeof(SmpRow) == 16, "one 16-byte load per row");

// Truncated sampling (fw_generate_trunc): the limits of the row's CALL, one entry per decode row, beside the SmpRow table and
// not inside it: SmpRow stays one 16-byte load for the kernels that never truncate, and only the TRUNC instantiations
// read this one (one uniform 8-byte load).  (0, 1.0): the row draws from its whole distribution.
struct TruncRow {
  int top_k;               // >= 0; 0: no limit
  float top_p;             // in (0, 1]; 1: no limit
};
static_assert(sizeof(TruncRow) == 8, "one 8-byte load per row");

// ptab != null (decode steps of a ragged run; ignored with an explicit position): [chunks] prompt length per chunk, the
// position of chunk c is min(ptab[c] - 1 + step, reach - 1) instead of P - 1 + step; kmul = rows per chunk
// blk_n > 0: POSITION BLOCKS (prompt forward, align) — the rows of a chunk are blk_n consecutive positions pos_fixed ..
// of its beam slot 0 (row = chunk * blk_n + j) instead of beams at one position; same per-row arithmetic, same bits
void launch_embed(hipStream_t st, const int* tok, const half_t* emb, const half_t* pos_emb, half_t* x, half_t* xfrag,
                  int rows, int d,
                  const int* d_step, int pos_fixed, int P, int blk_n = 0,
                  const int* ptab = nullptr, int kmul = 0, int reach = 0);
// whether launch_self_attn's second form (forms 2 / 3, and with it position blocks) is usable for this cache geometry
bool self_attn_block_ok(int n_ctx, int cache_ctx, int d, int R_total);
// the form (1 / 2 / 3, below) launch_self_attn takes for `chunks` workgroups per head under knob value `knob`; pure
int self_attn_form(int n_ctx, int cache_ctx, int d, int R_total, int kmul, int H, int chunks, int knob);
// n_ctx: stride of the slot table (the text context); cache_ctx: positions per slot of the K/V cache of this run
void launch_self_attn(hipStream_t st, const half_t* qkv, int d, half_t* kc, half_t* vc, int n_ctx, int cache_ctx, int H,
                      const uint8_t* kvidx2, int Kbeam, int kmul, half_t* out, int rows, const int* d_step,
                      int pos_fixed, int P, int R_total, int frag, int blk_n = 0, const int* ptab = nullptr,
                      int reach = 0);
// 0: the product's choice by launch size; 1: the first form (rounds 1-4); 2: latency form; 3: throughput form (same bits)
void set_self_attn_form(int form);
void set_cross_attn_regs(int cap);   // fw_test_knob(7, ..): register cap of dec_cross_attn_kernel (0 none, 1: 96, 2: 80)
// changes whenever a measurement knob changed the kernels a decode step launches: cached step graphs carry it
int kernel_forms_epoch();
void bump_kernel_forms_epoch();
// slot_map: [B / kv_div] encoder chunk of the run -> chunk slot behind ck / cvt (the cross-attention pool)
void launch_cross_attn(hipStream_t st, const half_t* qx, int d, const half_t* ck, const half_t* cvt, int T, int kvp,
                       int kmul, half_t* out, int B, int H, const int* done, int kv_div, int frag, const int* slot_map);
// rows from which a decode run's linears take the GEMM-shaped kernel (read from dec_linear_plan's table)
int dec_big_min_rows();
int dec_big_min_rows_of(int role, int compute_type);   // role 0 qkv, 1 d x d, 2 ffn1, 3 ffn2, < 0: the lowest; 0 fp16 / 1 int8
// Which kernel form a decoder linear takes: the numbers fw_test_dec_linear / fw_bench_dec_linear_epi pass through.
enum DecLinForm {
  DEC_LIN_PRODUCT = 0,       // the product's choice by shape and row count
  DEC_LIN_SKINNY = 5,        // the register-streaming (skinny) kernel whatever the row count
  DEC_LIN_SKINNY_1X1 = 6,    // ... with one 16 x 16 tile per workgroup
  DEC_LIN_SKINNY_2X2 = 7,    // ... with 2 x 2 tiles per workgroup
  DEC_LIN_BIG = 10,          // + cfg (0..2): the GEMM-shaped kernel of merged runs, workgroup shape cfg (dec_kernels.hip)
};
enum DecLinFamily { DEC_LIN_REFUSED = 0, DEC_LIN_FAMILY_SKINNY = 1, DEC_LIN_FAMILY_BIG = 2 };
struct DecLinPlan {
  int family;                       // DecLinFamily; the int8 kernel (compute_type 1) counts as skinny
  int cfg;                          // big: 0..2, else -1
  int row_tiles, col_tiles, chunk;  // skinny: 16 x 16 tiles per workgroup, k-steps of loads in flight per wave
  int waves;                        // 4 | 8: the waves K is split over = the K slice count of the big kernel
};
// THE place that decides the form of a decoder linear of R rows, [N][K] weights, output / residual row strides ldo / ldr
// (ldr = 0: no residual).  Arithmetic only: no HIP call, no lock, no allocation.  Every form returns the same bits.
DecLinPlan dec_linear_plan(int R, int N, int K, int ldo, int ldr, int compute_type, int form);
// xf / Wf fragment-major [rows/16][K/32][64][8] (what frag = 1 of the row kernels and launch_self_attn write); out
// (row-major) and out_frag (fragment-major, for the next linear) are both optional; res is row-major; s1 / cf: the
// LayerNorm-folded form (then bias is folded into cf)
struct DecLin {
  const half_t *xf, *Wf, *bias; const float *s1, *cf;
  const half_t* res; int ldr; half_t* out; int ldo; half_t* out_frag;
  int R, N, K, act;
};
// launches what dec_linear_plan says; -1 when the plan refuses (a forced form that does not fit, a shape no form takes)
int launch_dec_linear(hipStream_t st, const DecLin& a, int form = DEC_LIN_PRODUCT);
int launch_dec_gemm_frag_variant(hipStream_t st, int variant, bool lnf, const half_t* xf, const half_t* Wf,
                                 const half_t* bias, const float* s1, const float* cf, half_t* out, int R, int N,
                                 int K);
int launch_dec_gemm_frag_i8(hipStream_t st, const int8_t* xq, const float* x_scale, const int8_t* Wq,
                            const float* w_scale, const half_t* bias, const half_t* res, int ldr, half_t* out, int ldo,
                            int R, int N, int K, int act);
// vocabulary projection -> float32 logits; operands fragment-major (Wf: ceil(N/16) column tiles, zero-padded)
int launch_dec_logits(hipStream_t st, bool i8, const void* xf, const float* x_scale, const void* Wf,
                      const float* w_scale, const float* s1, const float* cf, float* out, int ldo, int R, int N, int K);
void launch_nospeech(hipStream_t st, const float* logits, int V, int row_mul, int no_speech_id, float* out, int B);
// sup_bits: the suppress list, one bit per token id, LP_SUP_WORDS 64-bit words (suppress_mask above)
// smp_tab [gp.R]: read when gp.sample (then it must not be null: the launcher launches nothing without it)
void launch_logits_process(hipStream_t st, const GenDev& gp, float* logits, const unsigned long long* sup_bits,
                           const int* hist2, const float* cum2, const int* d_step, const int* done, float* cand_val,
                           int* cand_tok, float* cand_lp = nullptr, const SmpRow* smp_tab = nullptr,
                           int* alt_tok = nullptr, float* alt_lp = nullptr, const TruncRow* trunc_tab = nullptr);
// TRUNC (gp.trunc != 0: sampling launches only, and trunc_tab [gp.R] must be given — otherwise nothing is launched): the
// TRUNC instantiations; a row whose entry is (0, 1.0) skips the stage and gets the bits of the plain sampling kernel.
// (the TRUNC launches themselves: dec_trunc.hip; called by launch_logits_process only)
void launch_logits_process_trunc(hipStream_t st, const GenDev& gp, float* logits, const unsigned long long* sup_bits,
                                 const int* hist2, const float* cum2, const int* d_step, const int* done, float* cand_val,
                                 int* cand_tok, float* cand_lp, const SmpRow* smp_tab, int* alt_tok, float* alt_lp,
                                 const TruncRow* trunc_tab);
// ALTERNATIVES (gp.n_alt > 0 and both alt pointers given, otherwise today's kernels): alt_tok / alt_lp [steps][gp.R][n_alt],
// row r at step s writes the first n_alt rounds of its extraction (log-prob descending, id ascending; (0, -inf) once
// nothing is left) to [s][r][.] — the registers cand_lp is written from; a sampling row runs n_alt plain rounds on the
// unperturbed log-probs after its draw.  fin_path [chunks][FIN_CAP][NT + 1] (beam update): for a finished hypothesis
// recorded at step s, byte q < s = the beam slot whose row produced token q (the source row's slot-table byte at
// Pc - 1 + q), byte s = the source row's own beam index: alt_*[q][c * K + fin_path[q]] belong to its tokens and to the step
// that closed it.  Nothing is copied per step.
// cand_lp [R][32]: the log-prob of every candidate (cand_val = cum + cand_lp), lphist2 [2][R][NT] the log-prob history
// beside hist2, fin_lp [.][FIN_CAP][NT + 1] the values of a finished hypothesis' tokens and, at [NT], of its <eot>.
// Null (all three of the beam update, or none): the kernels skip these stores.
void launch_beam_update(hipStream_t st, const GenDev& gp, const float* cand_val, const int* cand_tok, int* hist2,
                        float* cum2, uint8_t* kvidx2, int* cur_tok, const int* d_step, int* done, int* n_done,
                        int* n_fin, int* fin_tok, int* fin_len, float* fin_score, float* fin_cum,
                        const float* cand_lp = nullptr, float* lphist2 = nullptr, float* fin_lp = nullptr,
                        const int* ptab = nullptr, uint8_t* fin_path = nullptr);
// One returned hypothesis for launch_alt_gather: decode chunk, finished slot, length, and the step whose row produced the
// closing <eot> (-1: cut at the budget, no closing step).
struct AltHyp { int chunk, fin, len, end; };
static_assert(sizeof(AltHyp) == 16, "one 16-byte load per hypothesis");
// out_tok / out_lp [n_hyp][T + 1][n_alt]: entry t < len = alt_*[t][chunk * K + fin_path[t]][.], entry T = those of step
// `end`; entries in [len, T), and entry T of a hypothesis without closing step, are (-1, 0).  R: rows of the run that
// filled alt_* (its step stride).  Every len <= T, end < steps of alt_*, path byte < K: the caller's to guarantee.
void launch_alt_gather(hipStream_t st, const int* alt_tok, const float* alt_lp, const uint8_t* fin_path, const AltHyp* hyps,
                       int n_hyp, int R, int K, int NT, int n_alt, int T, int* out_tok, float* out_lp);
// ragged runs: rows of the final hidden state at each chunk's <sot> position -> row `chunk` of xo (row-major) and xof
// (fragment-major); nb > 0: a prompt pass over positions pos0 .. (row = chunk * nb + j), nb == 0: decode step 0
void launch_gather_sot_rows(hipStream_t st, const half_t* x, const int* sot_tab, const int* ptab, int pos0, int nb,
                            int rows_per_chunk, half_t* xo, half_t* xof, int d, int B);
void launch_step_advance(hipStream_t st, int* d_step);
// row b reads logits row b * row_mul
void launch_token_prob(hipStream_t st, const float* logits, int V, const int* target, float* out, int out_stride,
                       int out_off, int rows, int row_mul = 1);
void launch_cross_probs(hipStream_t st, const half_t* qx, int d, const half_t* ck, int T, int kvp, const int* heads,
                        int n_layer_heads, int n_sel, float* probs, int n_tok, int tok_idx, int B, int blk_n = 0);
// Scoring (fw_score): what one logits row is scored against.  target < 0: the row has no target, nothing is written.
struct ScoreRow {
  int target;              // the id whose log-prob is wanted
  int n;                   // tokens in front of it: the row's history is hist_pool[hist_off .. hist_off + n)
  int hist_off;
  int out;                 // index into out_lp / out_best_id / out_best_lp
};
static_assert(sizeof(ScoreRow) == 16, "one 16-byte load per row");
// row r of a score-form launch: position pos0 + r % nb of sequence r / nb (dec_score_kernel and the score forms of the two
// pre-pass kernels address their rows through this)
static __device__ __forceinline__ ScoreRow score_row(const ScoreRow* __restrict__ tab, int tab_stride, int pos0, int nb, int r) {
  const int sq = r / nb;
  return tab[(size_t)sq * tab_stride + pos0 + (r - sq * nb)];
}
// Where a pre-pass kernel (dec_boost_kernel, dec_constrain_kernel) finds its rows' histories.  Decode-step form: hist is
// hist2 [2][R][NT], d_step and done are the run's.  Score form: hist is the history pool, tab .. nb address the ScoreRows.
struct RowSource {
  const int* hist;
  const int* d_step;
  const int* done;
  const ScoreRow* tab;
  int tab_stride, pos0, nb;
};
// Row r's history hist[0 .. n), n clamped to NT.  False: the row is skipped (its chunk is done / it has no target); the
// answer is the same for every thread of the workgroup, and the caller returns on it before any barrier.
template <bool SCORE>
static __device__ __forceinline__ bool row_history(const RowSource& s, int r, int K, int R, int NT, const int*& hist, int& n) {
  if (SCORE) {
    const ScoreRow row = score_row(s.tab, s.tab_stride, s.pos0, s.nb, r);
    if (row.target < 0) return false;
    n = row.n;
    hist = s.hist + row.hist_off;
  } else {
    if (s.done[r / K]) return false;
    const int step = *s.d_step;
    n = step;   // tokens generated so far on this row
    hist = s.hist + ((size_t)(step & 1) * R + r) * NT;
  }
  n = n < NT ? n : NT;
  return true;
}
// dec_score_kernel over `rows` logits rows in ONE launch: row r is position pos0 + r % nb of sequence r / nb and reads
// tab[(r / nb) * tab_stride + pos0 + r % nb].  rules: the decoding rules of gp (with_ts, suppress_blank, mits, ngram,
// rep_pen, the token ids) and sup_bits first, on a greedy row whose history is the ScoreRow's; otherwise the raw
// distribution (sup_bits and hist_pool are not read).  The logits are not written.  Every id (targets, histories) must lie
// in [0, gp.V) and every n below LP_THREADS: the caller checks.  out_best_id / out_best_lp: both or neither.
void launch_score(hipStream_t st, const GenDev& gp, bool rules, const float* logits, const unsigned long long* sup_bits,
                  const ScoreRow* tab, int tab_stride, int pos0, int nb, int rows, const int* hist_pool, float* out_lp,
                  int* out_best_id, float* out_best_lp);

// ---- phrase boosting (include/fwamd.h: fw_boost; kernel and table compiler: dec_boost.hip) ----
// The compiled table, 32-bit words: a header {G groups, E entries, T phrase tokens, n_vocab}, then
//   grp_id [G]      the target ids, ascending: one group per distinct id some phrase holds
//   grp_off [G + 1] group g owns entries grp_off[g] .. grp_off[g + 1]
//   ent [E][3]      one per pair (j, k): {start of phrase j in tok, k, the bits of boosts[j]}; target id = tok[start + k]
//   tok [T]         the phrases back to back
// E == T (every token of every phrase is the target of exactly one pair), G <= E <= FW_BOOST_MAX_TOKENS.
constexpr int BOOST_HDR_WORDS = 4;
constexpr int BOOST_TABLE_MAX_WORDS = BOOST_HDR_WORDS + 2 * FW_BOOST_MAX_TOKENS + 1 + 3 * FW_BOOST_MAX_TOKENS + FW_BOOST_MAX_TOKENS;
struct BoostView {
  int G, E, T;
  const int *grp_id, *grp_off, *ent, *tok;
};
static __host__ __device__ inline BoostView boost_view(const int* tab) {
  BoostView v;
  v.G = tab[0]; v.E = tab[1]; v.T = tab[2];
  v.grp_id = tab + BOOST_HDR_WORDS;
  v.grp_off = v.grp_id + v.G;
  v.ent = v.grp_off + v.G + 1;
  v.tok = v.ent + 3 * v.E;
  return v;
}
// dec_boost_kernel, decode-step form, in front of launch_logits_process: row r of gp.R rows reads its history from the
// parity half of hist2 that *d_step selects (n = step), rows of chunks with done[r / gp.K] are skipped.  logits [gp.R][gp.V]
// IN / OUT: logits[r][v] += boost(v) for the ids with a matching pair, every other value keeps its bits.
void launch_boost_step(hipStream_t st, const GenDev& gp, float* logits, const int* boost_tab, const int* hist2,
                       const int* d_step, const int* done);
// ... score form, in front of launch_score, same row addressing: rows without a target (target < 0) are skipped, the
// history is the ScoreRow's.  Every n <= n_text_ctx, every table built by fw_boost_create for gp.V: the caller's to guarantee.
void launch_boost_score(hipStream_t st, const GenDev& gp, float* logits, const int* boost_tab, const ScoreRow* tab,
                        int tab_stride, int pos0, int nb, int rows, const int* hist_pool);
// the same walk in plain C++ (fw_test_boost_rows_host): row r's history is hist[hist_offsets[r] .. hist_offsets[r + 1])
void boost_rows_host(const int* boost_tab, float* logits, int rows, int V, const int* hist, const int* hist_offsets);

// ---- constrained decoding (include/fwamd.h: fw_constraint; kernel and table compiler: dec_constrain.hip) ----
// The compiled table, 32-bit words: a header {P phrases, T phrase tokens, n_vocab, 0}, then
//   off [P + 1]     phrase j is tok[off[j] .. off[j + 1]), off[0] = 0
//   tok [T]         the phrases back to back
// The phrases are a set: sorted by their ids (lexicographically), no duplicates.  P <= FW_CONSTRAIN_MAX_PHRASES,
// T <= FW_CONSTRAIN_MAX_TOKENS, every phrase 1 .. FW_CONSTRAIN_MAX_LEN tokens.
constexpr int CONSTRAIN_HDR_WORDS = 4;
constexpr int CONSTRAIN_TABLE_MAX_WORDS = CONSTRAIN_HDR_WORDS + FW_CONSTRAIN_MAX_PHRASES + 1 + FW_CONSTRAIN_MAX_TOKENS;
struct ConstrainView {
  int P, T;
  const int *off, *tok;
};
static __host__ __device__ inline ConstrainView constrain_view(const int* tab) {
  ConstrainView v;
  v.P = tab[0]; v.T = tab[1];
  v.off = tab + CONSTRAIN_HDR_WORDS;
  v.tok = v.off + v.P + 1;
  return v;
}
// dec_constrain_kernel, decode-step form, behind launch_boost_step and in front of launch_logits_process: row r of gp.R
// rows reads its history from the parity half of hist2 that *d_step selects (n = step), rows of chunks with
// done[r / gp.K] are skipped.  logits [gp.R][gp.V] IN / OUT: every text id (< gp.ts_begin) that no phrase allows after the
// row's history (include/fwamd.h) becomes -inf, gp.eot included unless the history is a whole phrase; the timestamp ids
// become -inf unless gp.with_ts; every other value keeps its bits, nothing is read.  Reads gp.V, K, R, n_text_ctx, eot,
// ts_begin, with_ts.  Nothing is launched unless 0 <= eot < ts_begin <= V <= 64 * LP_SUP_WORDS: the callers check.
void launch_constrain_step(hipStream_t st, const GenDev& gp, float* logits, const int* constrain_tab, const int* hist2,
                           const int* d_step, const int* done);
// ... score form, in front of launch_score, same row addressing: rows without a target (target < 0) are skipped, the
// history is the ScoreRow's.  Every n <= n_text_ctx, a table built by fw_constraint_create: the caller's to guarantee.
void launch_constrain_score(hipStream_t st, const GenDev& gp, float* logits, const int* constrain_tab, const ScoreRow* tab,
                            int tab_stride, int pos0, int nb, int rows, const int* hist_pool);
// the same walk in plain C++ (fw_test_constrain_rows_host): row r's history is hist[hist_offsets[r] .. hist_offsets[r + 1])
void constrain_rows_host(const int* constrain_tab, float* logits, int rows, int V, int eot, int ts_begin, int with_ts,
                         const int* hist, const int* hist_offsets);

}  // namespace fwd

// What fw_boost and fw_constraint share: the list's vocabulary size and its compiled table (above).  An empty list (first
// header word 0) is no list, and a decode run walks ONE table per kind: the rules the decode path asks of either kind
// are stated once here.
struct fw_phrase_table {
  int32_t n_vocab;
  std::vector<int32_t> table;
};
namespace fwd {
static inline bool phrase_list_live(const fw_phrase_table* t) { return t && t->table[0] > 0; }
// both none, or one table (the same list, or lists that compiled to the same bytes)
static inline bool phrase_table_same(const fw_phrase_table* a, const fw_phrase_table* b) {
  return a == b || (a && b && a->table == b->table);
}
// what both *_create functions ask of (n_vocab, tokens, offsets, n_phrases), against the kind's three limits
int32_t phrase_list_check(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases, int max_phrases,
                          int max_len, int max_tokens);
}  // namespace fwd

// what fw_boost_create returns
struct fw_boost : fw_phrase_table {};

// what fw_constraint_create returns: with, per compiled phrase, the index the caller gave its first occurrence (for
// messages only: never compared)
struct fw_constraint : fw_phrase_table {
  std::vector<int32_t> first;
};
