// Constrained decoding (include/fwamd.h: fw_constraint) for gfx950: the table compiler (host), dec_constrain_kernel — which
// sets every id of a row of float32 logits that the phrase list does not allow to -inf, behind the boost and in front of the
// rules kernel (decode steps) or the scoring kernel — and the same walk in plain C++.  What one phrase allows after one
// history is ONE function below, called by the kernel's two row forms and by the host walk.
#include "engine.h"

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <new>

#include "dec_kernels.h"

namespace fwd {

// What phrase j allows on a row whose history WITHOUT its timestamp ids is t[0 .. m): nothing (-1) when the phrase is
// shorter than m or differs from t somewhere, `eot` when the phrase is t, its token m otherwise.  Reads t[0 .. min(m, L_j)):
// the caller holds the first FW_CONSTRAIN_MAX_LEN + 1 text ids, and m beyond that matches no phrase.
static __host__ __device__ __forceinline__ int constrain_next(const ConstrainView& cv, int j, const int* t, int m, int eot) {
  const int start = cv.off[j], L = cv.off[j + 1] - start;
  if (m > L) return -1;
  const int* p = cv.tok + start;
  for (int q = 0; q < m; ++q)
    if (p[q] != t[q]) return -1;
  return m < L ? p[m] : eot;
}

// bit v of the row's keep mask as it starts out: the timestamp ids when the timestamp rules are on, nothing else
static __host__ __device__ __forceinline__ unsigned constrain_word_init(int w, int ts_begin, int with_ts) {
  const int lo = w * 32;
  if (!with_ts || lo + 32 <= ts_begin) return 0u;
  return lo >= ts_begin ? ~0u : ~0u << (ts_begin - lo);
}

}  // namespace fwd

// ------------------------------------------------------------------------------------
// dec_constrain_kernel: one workgroup per logits row, three phases with workgroup barriers between them.
//   1. the row's history without its timestamp ids, compacted in order into LDS (ballot + popcount per wave, the wave
//      totals through LDS); only the first FW_CONSTRAIN_MAX_LEN + 1 are kept, m counts on to at least that;
//   2. a keep mask of one bit per id in LDS: the timestamp ids when the rules want them, then threads stride over the
//      phrases and OR in what each allows (LDS atomics on a bit: the mask does not depend on the order);
//   3. -inf over every id whose bit is clear.  The logits are never read: a group of four ids with no bit set takes ONE
//      16-byte store, a mixed group one 4-byte store per cleared id, a kept id none — its bits are untouched.  The row
//      starts at r * V floats, 16-, 4-, 8- or 12-byte aligned: up to three ids in front of the first 16-byte boundary and
//      up to three behind the last are peeled off in plain stores, no store is wider than its alignment.
// SCORE = false, the decode step: the history is the parity half of hist2 that *d_step selects, n = step, rows of done
// chunks return.  SCORE = true: row r is position pos0 + r % nb of sequence r / nb, as dec_score_kernel addresses it; a row
// without a target returns.
// ------------------------------------------------------------------------------------
#define CONSTRAIN_THREADS 256
#define CONSTRAIN_WAVES (CONSTRAIN_THREADS / 64)
// (one word more than the ids need: the 64-bit window of the last group reads it)
#define CONSTRAIN_MASK_WORDS (LP_SUP_WORDS * 2 + 1)
template <bool SCORE>
__global__ __launch_bounds__(CONSTRAIN_THREADS) void dec_constrain_kernel(
    float* __restrict__ logits, const int* __restrict__ ctab, int V, int K, int R, int NT, int eot, int ts_begin, int with_ts,
    fwd::RowSource src) {
  __shared__ unsigned keep[CONSTRAIN_MASK_WORDS];
  __shared__ int text[FW_CONSTRAIN_MAX_LEN + 1];
  __shared__ int wave_n[CONSTRAIN_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform, in front of the first barrier)

  // 1. the text ids of the history, in order
  int m = 0;
  for (int i0 = 0; i0 < n && m <= FW_CONSTRAIN_MAX_LEN; i0 += CONSTRAIN_THREADS) {   // (uniform)
    const int i = i0 + tid;
    const int id = i < n ? hist[i] : ts_begin;
    const bool is_text = id < ts_begin;
    const unsigned long long b = __ballot(is_text);
    if (lane == 0) wave_n[wv] = __popcll(b);
    __syncthreads();
    int pos = m + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < CONSTRAIN_WAVES; ++w) {
      pos += w < wv ? wave_n[w] : 0;
      total += wave_n[w];
    }
    if (is_text && pos <= FW_CONSTRAIN_MAX_LEN) text[pos] = id;
    m += total;
    __syncthreads();
  }

  // 2. the keep mask
  const int n_words = (V + 31) / 32 + 1;
  for (int w = tid; w < n_words; w += CONSTRAIN_THREADS) keep[w] = fwd::constrain_word_init(w, ts_begin, with_ts);
  __syncthreads();
  if (m <= FW_CONSTRAIN_MAX_LEN) {
    const fwd::ConstrainView cv = fwd::constrain_view(ctab);
    for (int j = tid; j < cv.P; j += CONSTRAIN_THREADS) {
      const int v = fwd::constrain_next(cv, j, text, m, eot);
      if (v >= 0 && v < ts_begin) atomicOr(&keep[v >> 5], 1u << (v & 31));   // (ts_begin <= V: inside the mask)
    }
  }
  __syncthreads();

  // 3. -inf over the rest
  const float NEG = -INFINITY;
  float* lg = logits + (size_t)r * V;
  int head = (int)(((16u - (unsigned)((uintptr_t)lg & 15u)) & 15u) >> 2);   // ids in front of the first 16-byte boundary
  head = head < V ? head : V;
  const int n_vec = (V - head) >> 2, tail0 = head + 4 * n_vec;
  if (tid < head && !((keep[tid >> 5] >> (tid & 31)) & 1u)) lg[tid] = NEG;
  {
    const int v = tail0 + tid;   // tid < 3 at most
    if (v < V && !((keep[v >> 5] >> (v & 31)) & 1u)) lg[v] = NEG;
  }
  const float4 neg4 = make_float4(NEG, NEG, NEG, NEG);
  for (int i = tid; i < n_vec; i += CONSTRAIN_THREADS) {
    const int v0 = head + 4 * i;   // v0 + 3 < tail0 <= V
    const int w = v0 >> 5;
    const unsigned long long win = ((unsigned long long)keep[w + 1] << 32) | keep[w];
    const unsigned k4 = (unsigned)(win >> (v0 & 31)) & 15u;
    if (k4 == 0u) {
      *reinterpret_cast<float4*>(lg + v0) = neg4;
    } else if (k4 != 15u) {
      if (!(k4 & 1u)) lg[v0] = NEG;
      if (!(k4 & 2u)) lg[v0 + 1] = NEG;
      if (!(k4 & 4u)) lg[v0 + 2] = NEG;
      if (!(k4 & 8u)) lg[v0 + 3] = NEG;
    }
  }
}

namespace fwd {

// what the kernel's mask holds: V ids, the token ids in order inside it
static bool constrain_geometry_ok(int V, int eot, int ts_begin) {
  return V >= 1 && V <= LP_SUP_WORDS * 64 && eot >= 0 && eot < ts_begin && ts_begin <= V;
}

void launch_constrain_step(hipStream_t st, const GenDev& gp, float* logits, const int* ctab, const int* hist2,
                           const int* d_step, const int* done) {
  if (!ctab || gp.R <= 0 || !constrain_geometry_ok(gp.V, gp.eot, gp.ts_begin)) return;
  dec_constrain_kernel<false><<<gp.R, CONSTRAIN_THREADS, 0, st>>>(logits, ctab, gp.V, gp.K, gp.R, gp.n_text_ctx, gp.eot,
                                                                 gp.ts_begin, gp.with_ts,
                                                                 {hist2, d_step, done, nullptr, 0, 0, 1});
}

void launch_constrain_score(hipStream_t st, const GenDev& gp, float* logits, const int* ctab, const ScoreRow* tab,
                            int tab_stride, int pos0, int nb, int rows, const int* hist_pool) {
  if (!ctab || rows <= 0 || !constrain_geometry_ok(gp.V, gp.eot, gp.ts_begin)) return;
  dec_constrain_kernel<true><<<rows, CONSTRAIN_THREADS, 0, st>>>(logits, ctab, gp.V, 1, rows, gp.n_text_ctx, gp.eot,
                                                                gp.ts_begin, gp.with_ts,
                                                                {hist_pool, nullptr, nullptr, tab, tab_stride, pos0, nb});
}

void constrain_rows_host(const int* ctab, float* logits, int rows, int V, int eot, int ts_begin, int with_ts, const int* hist,
                         const int* hist_offsets) {
  if (!constrain_geometry_ok(V, eot, ts_begin)) return;
  const ConstrainView cv = constrain_view(ctab);
  std::vector<unsigned> keep((size_t)(V + 31) / 32);
  for (int r = 0; r < rows; ++r) {
    int text[FW_CONSTRAIN_MAX_LEN + 1], m = 0;
    for (int i = hist_offsets[r]; i < hist_offsets[r + 1]; ++i) {
      if (hist[i] >= ts_begin) continue;
      if (m <= FW_CONSTRAIN_MAX_LEN) text[m] = hist[i];
      ++m;
    }
    for (size_t w = 0; w < keep.size(); ++w) keep[w] = constrain_word_init((int)w, ts_begin, with_ts);
    if (m <= FW_CONSTRAIN_MAX_LEN)
      for (int j = 0; j < cv.P; ++j) {
        const int v = constrain_next(cv, j, text, m, eot);
        if (v >= 0 && v < ts_begin) keep[v >> 5] |= 1u << (v & 31);
      }
    float* lg = logits + (size_t)r * V;
    for (int v = 0; v < V; ++v)
      if (!((keep[v >> 5] >> (v & 31)) & 1u)) lg[v] = -INFINITY;
  }
}

}  // namespace fwd

extern "C" {

int32_t fw_constraint_create(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
                             fw_constraint** out) {
  FW_CHECK_ARG(out, "null argument");
  *out = nullptr;
  if (int rc = fwd::phrase_list_check(n_vocab, tokens, offsets, n_phrases, FW_CONSTRAIN_MAX_PHRASES, FW_CONSTRAIN_MAX_LEN,
                                      FW_CONSTRAIN_MAX_TOKENS))
    return rc;
  // The list is a SET of phrases: sorted by their ids, duplicates dropped — lists that hold the same phrases give the same
  // bytes in whatever order and however often they name them.  `first` keeps, per compiled phrase, the caller's index of
  // its first occurrence (for messages; not part of the table).
  std::vector<int> order((size_t)n_phrases);
  for (int j = 0; j < n_phrases; ++j) order[j] = j;
  const auto less = [&](int a, int b) {
    return std::lexicographical_compare(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b], tokens + offsets[b + 1]);
  };
  std::stable_sort(order.begin(), order.end(), less);   // (stable: equal phrases stay in the caller's order)
  fw_constraint* c = new (std::nothrow) fw_constraint();
  if (!c) { fw::set_error("out of host memory"); return FW_ENOMEM; }
  c->n_vocab = n_vocab;
  std::vector<int32_t> off(1, 0), tok;
  for (int i = 0; i < n_phrases; ++i) {
    const int j = order[i];
    if (i > 0 && !less(order[i - 1], j)) continue;   // (sorted: not less means equal)
    tok.insert(tok.end(), tokens + offsets[j], tokens + offsets[j + 1]);
    off.push_back((int32_t)tok.size());
    c->first.push_back(j);
  }
  std::vector<int32_t>& tab = c->table;
  tab.reserve((size_t)fwd::CONSTRAIN_HDR_WORDS + off.size() + tok.size());
  tab.push_back((int32_t)c->first.size()); tab.push_back((int32_t)tok.size()); tab.push_back(n_vocab); tab.push_back(0);
  tab.insert(tab.end(), off.begin(), off.end());
  tab.insert(tab.end(), tok.begin(), tok.end());
  *out = c;
  return FW_OK;
}

void fw_constraint_free(fw_constraint* c) { delete c; }

}  // extern "C"
