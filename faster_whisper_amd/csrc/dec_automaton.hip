// Automaton-constrained decoding (include/fwamd.h: fw_automaton) for gfx950: the table compiler (host), dec_automaton_kernel —
// which sets every id of a row of float32 logits that the automaton does not allow after the row's history to -inf, behind
// the boost and in front of the rules kernel (decode steps) or the scoring kernel — and the same walk in plain C++.  The
// table layout (one record per state, a state is its record's offset): dec_kernels.h.
#include "engine.h"

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <new>

#include "dec_kernels.h"

// ------------------------------------------------------------------------------------
// dec_automaton_kernel: one workgroup of four waves per logits row.
//   1. COMPACTION.  The row's history without its timestamp ids, in order, into LDS: ballot + popcount per wave, the wave
//      totals through LDS — the constraint's scheme without its 33-id cap, up to n_text_ctx <= AUTOMATON_MAX_HIST ids.
//   2. STAGING.  The walk below is a chain of m dependent table fetches, so where the table lives sets the kernel's time.
//      A row with at least stage_min text ids (header word 3: automaton_stage_min) copies the whole table into LDS first —
//      all four waves, 16-byte loads — and walks it there; a shorter history walks the table where it lies (L2).  The
//      kernel comes with two LDS allocations (LDSW words): tables of up to AUTOMATON_LDS_SMALL_WORDS take the small one
//      (three workgroups per CU), larger ones the large one (about 110 KB with the mask: one workgroup per CU).  A table
//      that does not fit its allocation is walked in L2: LDS is never overrun.
//   3. THE WALK, by wave 0 alone, while waves 1 .. 3 initialise the keep mask (the timestamp ids when the rules want them).
//      A transition is ONE wave-wide fetch: the 64 lanes load the state's first 64 (token, target) pairs in one coalesced
//      8-byte-per-lane read — the record's edge count is loaded beside it, not in front of it — a ballot finds the lane
//      whose token is the history id, a readlane of that lane's target is the next state.  The state stays in a scalar
//      register throughout.  A state of more than 64 edges takes one fetch more: lane c loads the LAST token of 64-pair
//      chunk c (the tokens ascend), the first chunk whose last token is >= the id is the only one that can hold it, and
//      that chunk is matched as above; 4096 edges per round, two rounds at FW_AUTOMATON_MAX_EDGES.  No edge: the history
//      has left the language, the walk ends with no state.
//   4. THE MASK.  After a barrier all threads OR the final state's edge tokens, and <eot> if it accepts, into the mask
//      (LDS atomics on a bit); without a state nothing is added.
//   5. -inf over every id whose bit is clear: fwd::write_neg_inf_row (dec_kernels.h), the constraint's writer.  The logits
//      are never read.
// SCORE = false / true: the two row forms of fwd::row_history, as dec_constrain_kernel has them.
// ------------------------------------------------------------------------------------
#define AUTOMATON_THREADS 256
#define AUTOMATON_WAVES (AUTOMATON_THREADS / 64)
// (one word more than the ids need: the 64-bit window of the writer's last group reads it)
#define AUTOMATON_MASK_WORDS (LP_SUP_WORDS * 2 + 1)

namespace fwd {

// the pair (token, target record) of lane `lane` in the 64-pair chunk that starts at pair `p0` of record `rec`: inside the
// table for every lane by its padding
static __device__ __forceinline__ int2 automaton_pair(const int* tab, int rec, int p0, int lane) {
  return *reinterpret_cast<const int2*>(tab + rec + 2 + 2 * (p0 + lane));
}

// delta*(start state, text[0 .. m)) as a record offset, -1 when undefined.  Called by ONE whole wave; the result is
// wave-uniform.  `tab` is the table in LDS or in global memory (inlined at both call sites, each with its address space).
static __device__ __forceinline__ int automaton_walk(const int* tab, const int* text, int m, int lane) {
  int rec = AUTOMATON_HDR_WORDS;
  for (int q = 0; q < m; ++q) {
    const int t = text[q];
    const int n = __builtin_amdgcn_readfirstlane(tab[rec]);
    int p0 = 0;
    if (n > 64) {   // (uniform) the chunk whose last token is the first one >= t
      const int n_chunks = (n + 63) >> 6;
      p0 = -1;
      for (int c0 = 0; c0 < n_chunks && p0 < 0; c0 += 64) {
        const int c = c0 + lane;
        const int last = min(64 * c + 63, n - 1);
        const bool ge = c < n_chunks && tab[rec + 2 + 2 * last] >= t;
        const unsigned long long b = __ballot(ge);
        if (b) p0 = 64 * (c0 + __ffsll((long long)b) - 1);
      }
      if (p0 < 0) return -1;   // t is above every token of the state
    }
    const int2 e = automaton_pair(tab, rec, p0, lane);
    const unsigned long long hit = __ballot(p0 + lane < n && e.x == t);
    if (!hit) return -1;
    rec = __builtin_amdgcn_readlane(e.y, __ffsll((long long)hit) - 1);
  }
  return rec;
}

}  // namespace fwd

template <bool SCORE, int LDSW>
__global__ __launch_bounds__(AUTOMATON_THREADS) void dec_automaton_kernel(
    float* __restrict__ logits, const int* __restrict__ atab, int V, int K, int R, int NT, int eot, int ts_begin, int with_ts,
    fwd::RowSource src) {
  __shared__ __attribute__((aligned(16))) int ltab[LDSW];
  __shared__ unsigned keep[AUTOMATON_MASK_WORDS];
  __shared__ int text[fwd::AUTOMATON_MAX_HIST];
  __shared__ int wave_n[AUTOMATON_WAVES];
  __shared__ int final_rec;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform, in front of the first barrier)
  n = n < fwd::AUTOMATON_MAX_HIST ? n : fwd::AUTOMATON_MAX_HIST;      // (the launchers refuse a longer text context)

  // 1. the text ids of the history, in order
  int m = 0;
  for (int i0 = 0; i0 < n; i0 += AUTOMATON_THREADS) {   // (uniform)
    const int i = i0 + tid;
    const int id = i < n ? hist[i] : ts_begin;
    const bool is_text = id < ts_begin;
    const unsigned long long b = __ballot(is_text);
    if (lane == 0) wave_n[wv] = __popcll(b);
    __syncthreads();
    int pos = m + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < AUTOMATON_WAVES; ++w) {
      pos += w < wv ? wave_n[w] : 0;
      total += wave_n[w];
    }
    if (is_text) text[pos] = id;   // (pos < n)
    m += total;
    __syncthreads();
  }

  // 2. the table into LDS, for a history long enough to pay for it
  const int words = fwd::automaton_table_words(atab[0], atab[1]);   // (a multiple of 4)
  const bool staged = m >= atab[3] && words <= LDSW;   // (uniform)
  if (staged) {
    const int4* g4 = reinterpret_cast<const int4*>(atab);
    int4* l4 = reinterpret_cast<int4*>(ltab);
    for (int i = tid; i < (words >> 2); i += AUTOMATON_THREADS) l4[i] = g4[i];
    __syncthreads();
  }

  // 3. wave 0 walks, the others start the mask
  if (wv == 0) {
    const int rec = staged ? fwd::automaton_walk(ltab, text, m, lane) : fwd::automaton_walk(atab, text, m, lane);
    if (lane == 0) final_rec = rec;
  } else {
    const int n_words = (V + 31) / 32 + 1;
    for (int w = tid - 64; w < n_words; w += AUTOMATON_THREADS - 64) keep[w] = fwd::constrain_word_init(w, ts_begin, with_ts);
  }
  __syncthreads();

  // 4. what the final state allows
  const int rec = final_rec;
  if (rec >= 0) {
    const int* tab = staged ? (const int*)ltab : atab;
    const int n_e = tab[rec];
    for (int i = tid; i < n_e; i += AUTOMATON_THREADS) {
      const int v = tab[rec + 2 + 2 * i];
      if (v >= 0 && v < ts_begin) atomicOr(&keep[v >> 5], 1u << (v & 31));   // (ts_begin <= V: inside the mask)
    }
    if (tid == 0 && tab[rec + 1]) atomicOr(&keep[eot >> 5], 1u << (eot & 31));
  }
  __syncthreads();

  // 5. -inf over the rest
  fwd::write_neg_inf_row(logits + (size_t)r * V, V, keep, tid, AUTOMATON_THREADS);
}

namespace fwd {

// the large allocation holds every table; with the mask and the history it stays below gfx950's 160 KB of LDS
constexpr int AUTOMATON_LDS_LARGE_WORDS = AUTOMATON_TABLE_MAX_WORDS;
static_assert((AUTOMATON_LDS_LARGE_WORDS + AUTOMATON_MASK_WORDS + AUTOMATON_MAX_HIST + 8) * 4 <= 160 * 1024, "LDS of gfx950");

// what the kernel's mask and history buffer hold
static bool automaton_geometry_ok(int V, int eot, int ts_begin, int n_text_ctx) {
  return V >= 1 && V <= LP_SUP_WORDS * 64 && eot >= 0 && eot < ts_begin && ts_begin <= V && n_text_ctx <= AUTOMATON_MAX_HIST;
}

// THE staging rule.  Measured on an MI355X at large-v3's vocabulary (profiles/automaton_cost.py; DESIGN.md has the table): a
// transition costs about 0.27 us in L2 and 0.16 us in LDS, staging about 2 us for a table of 16 K words and 3 us for the
// largest at 80 rows (more at a full lane, where the large allocation leaves one workgroup per CU).  The walks break even
// near 16 ids for the phrase-list table and between 16 and 64 for the largest: 8 ids plus one per 1024 table words.
int automaton_stage_min(size_t table_words) { return 8 + (int)(table_words / 1024); }

template <bool SCORE>
static void launch_automaton_form(hipStream_t st, const GenDev& gp, float* logits, const int* atab, const RowSource& src,
                                  int K, int R) {
  if (gp.automaton == 1)
    dec_automaton_kernel<SCORE, AUTOMATON_LDS_SMALL_WORDS><<<R, AUTOMATON_THREADS, 0, st>>>(
        logits, atab, gp.V, K, R, gp.n_text_ctx, gp.eot, gp.ts_begin, gp.with_ts, src);
  else
    dec_automaton_kernel<SCORE, AUTOMATON_LDS_LARGE_WORDS><<<R, AUTOMATON_THREADS, 0, st>>>(
        logits, atab, gp.V, K, R, gp.n_text_ctx, gp.eot, gp.ts_begin, gp.with_ts, src);
}

void launch_automaton(hipStream_t st, const GenDev& gp, float* logits, const int* atab, const RowSource& src, int rows) {
  const bool step = src.tab == nullptr;
  if (!atab || (step ? gp.R : rows) <= 0 || !automaton_geometry_ok(gp.V, gp.eot, gp.ts_begin, gp.n_text_ctx)) return;
  if (step) launch_automaton_form<false>(st, gp, logits, atab, src, gp.K, gp.R);
  else launch_automaton_form<true>(st, gp, logits, atab, src, 1, rows);
}

int automaton_next_host(const int* tab, int rec, int token) {
  const int n = tab[rec];
  const int* pairs = tab + rec + 2;
  int lo = 0, hi = n;   // the tokens ascend: the first pair whose token is >= `token`
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (pairs[2 * mid] < token) lo = mid + 1; else hi = mid;
  }
  return lo < n && pairs[2 * lo] == token ? pairs[2 * lo + 1] : -1;
}

void automaton_rows_host(const int* tab, float* logits, int rows, int V, int eot, int ts_begin, int with_ts, const int* hist,
                         const int* hist_offsets) {
  if (!automaton_geometry_ok(V, eot, ts_begin, 0)) return;
  std::vector<unsigned> keep((size_t)(V + 31) / 32);
  for (int r = 0; r < rows; ++r) {
    int rec = AUTOMATON_HDR_WORDS;
    for (int i = hist_offsets[r]; i < hist_offsets[r + 1] && rec >= 0; ++i)
      if (hist[i] < ts_begin) rec = automaton_next_host(tab, rec, hist[i]);
    for (size_t w = 0; w < keep.size(); ++w) keep[w] = constrain_word_init((int)w, ts_begin, with_ts);
    if (rec >= 0) {
      for (int i = 0; i < tab[rec]; ++i) {
        const int v = tab[rec + 2 + 2 * i];
        if (v >= 0 && v < ts_begin) keep[v >> 5] |= 1u << (v & 31);
      }
      if (tab[rec + 1]) keep[eot >> 5] |= 1u << (eot & 31);
    }
    float* lg = logits + (size_t)r * V;
    for (int v = 0; v < V; ++v)
      if (!((keep[v >> 5] >> (v & 31)) & 1u)) lg[v] = -INFINITY;
  }
}

// the states `from` reaches along `next` (a CSR adjacency: forward edges, or the reversed ones)
static std::vector<char> automaton_reach(int n_states, const std::vector<int>& from, const std::vector<int32_t>& off,
                                         const std::vector<int32_t>& next) {
  std::vector<char> seen((size_t)n_states, 0);
  std::vector<int> stack(from);
  for (int s : from) seen[s] = 1;
  while (!stack.empty()) {
    const int s = stack.back();
    stack.pop_back();
    for (int i = off[s]; i < off[s + 1]; ++i)
      if (!seen[next[i]]) { seen[next[i]] = 1; stack.push_back(next[i]); }
  }
  return seen;
}

}  // namespace fwd

extern "C" {

int32_t fw_automaton_create(int32_t n_vocab, int32_t n_states, const int32_t* edge_offsets, const int32_t* edge_tokens,
                            const int32_t* edge_targets, const int32_t* accepting, fw_automaton** out) {
  FW_CHECK_ARG(out, "null argument");
  *out = nullptr;
  FW_CHECK_ARG(n_vocab >= 1, "n_vocab %d must be positive", n_vocab);
  FW_CHECK_ARG(edge_offsets && edge_tokens && edge_targets && accepting, "null argument");
  FW_CHECK_ARG(n_states >= 1 && n_states <= FW_AUTOMATON_MAX_STATES, "%d states not in [1, %d]", n_states,
               FW_AUTOMATON_MAX_STATES);
  FW_CHECK_ARG(edge_offsets[0] == 0, "edge_offsets[0] = %d, not 0", edge_offsets[0]);
  for (int s = 0; s < n_states; ++s) {
    FW_CHECK_ARG(edge_offsets[s + 1] >= edge_offsets[s], "edge_offsets decrease at state %d", s);
    FW_CHECK_ARG(edge_offsets[s + 1] <= FW_AUTOMATON_MAX_EDGES, "more than %d edges (at state %d)", FW_AUTOMATON_MAX_EDGES, s);
  }
  const int E = edge_offsets[n_states];
  for (int s = 0; s < n_states; ++s)
    for (int i = edge_offsets[s]; i < edge_offsets[s + 1]; ++i) {
      const int t = edge_tokens[i], to = edge_targets[i];
      FW_CHECK_ARG(t >= 0 && t < n_vocab, "state %d: edge id %d outside [0, %d)", s, t, n_vocab);
      FW_CHECK_ARG(to >= 0 && to < n_states, "state %d, id %d: target %d outside [0, %d)", s, t, to, n_states);
      FW_CHECK_ARG(i == edge_offsets[s] || edge_tokens[i - 1] < t,
                   "state %d: id %d follows id %d — a state's edge ids must ascend strictly (one edge per id)", s, t,
                   edge_tokens[i - 1]);
    }
  // trim: every state reachable from state 0, an accepting state reachable from every state
  const std::vector<int32_t> off(edge_offsets, edge_offsets + n_states + 1), to(edge_targets, edge_targets + E);
  const std::vector<char> fwd_seen = fwd::automaton_reach(n_states, {0}, off, to);
  for (int s = 0; s < n_states; ++s) FW_CHECK_ARG(fwd_seen[s], "state %d cannot be reached from state 0", s);
  std::vector<int32_t> roff((size_t)n_states + 1, 0), rto((size_t)E);
  for (int i = 0; i < E; ++i) ++roff[to[i] + 1];
  for (int s = 0; s < n_states; ++s) roff[s + 1] += roff[s];
  {
    std::vector<int32_t> fill(roff.begin(), roff.end() - 1);
    for (int s = 0; s < n_states; ++s)
      for (int i = off[s]; i < off[s + 1]; ++i) rto[fill[to[i]]++] = s;
  }
  std::vector<int> acc;
  for (int s = 0; s < n_states; ++s)
    if (accepting[s]) acc.push_back(s);
  const std::vector<char> bwd_seen = fwd::automaton_reach(n_states, acc, roff, rto);
  for (int s = 0; s < n_states; ++s) FW_CHECK_ARG(bwd_seen[s], "no accepting state can be reached from state %d", s);

  fw_automaton* a = new (std::nothrow) fw_automaton();
  if (!a) { fw::set_error("out of host memory"); return FW_ENOMEM; }
  a->n_vocab = n_vocab;
  std::vector<int32_t> rec((size_t)n_states);
  int32_t at = fwd::AUTOMATON_HDR_WORDS;
  for (int s = 0; s < n_states; ++s) { rec[s] = at; at += 2 + 2 * (off[s + 1] - off[s]); }
  const size_t words = (size_t)fwd::automaton_table_words(n_states, E);   // (>= at + AUTOMATON_PAD_WORDS)
  std::vector<int32_t>& tab = a->table;
  tab.reserve(words);
  tab.push_back(n_states); tab.push_back(E); tab.push_back(n_vocab); tab.push_back(fwd::automaton_stage_min(words));
  for (int s = 0; s < n_states; ++s) {
    tab.push_back(off[s + 1] - off[s]);
    tab.push_back(accepting[s] ? 1 : 0);
    for (int i = off[s]; i < off[s + 1]; ++i) { tab.push_back(edge_tokens[i]); tab.push_back(rec[to[i]]); }
  }
  tab.resize(words, -1);
  *out = a;
  return FW_OK;
}

void fw_automaton_free(fw_automaton* a) { delete a; }

}  // extern "C"
