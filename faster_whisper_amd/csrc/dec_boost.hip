// Phrase boosting (include/fwamd.h: fw_boost) for gfx950: the table compiler (host), dec_boost_kernel — which adds the
// boosts to a row of float32 logits in front of the rules kernel (decode steps) or the scoring kernel — and the same walk in
// plain C++.  The match of one target id against one history is ONE function below, called by the kernel's two row forms and
// by the host walk.
#include "engine.h"

#include <math.h>

#include <algorithm>
#include <new>

#include "dec_kernels.h"

namespace fwd {

// The boost of the id that owns entries e0 .. e1 of `tv`, on a row whose generated history is hist[0 .. n): the maximum
// boost over the entries (start, k, boost) whose k-token prefix tok[start .. start + k) equals hist[n - k .. n).  k > n never
// matches (nothing in front of hist[0] is read); k = 0 always does.  Compared from the newest token back: a prefix that
// differs anywhere ends the entry at its first differing token.  Returns whether any entry matched.
static __host__ __device__ __forceinline__ bool boost_of_group(const BoostView& tv, int e0, int e1, const int* hist, int n,
                                                               float& boost) {
  bool any = false;
  float best = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int start = tv.ent[3 * e], k = tv.ent[3 * e + 1];
    if (k > n) continue;
    const int* p = tv.tok + start;
    const int* h = hist + (n - k);
    bool match = true;
    for (int q = k - 1; q >= 0; --q)
      if (h[q] != p[q]) { match = false; break; }
    if (!match) continue;
    const float b = __builtin_bit_cast(float, tv.ent[3 * e + 2]);
    best = (!any || b > best) ? b : best;   // (fp32 max over finite values)
    any = true;
  }
  boost = best;
  return any;
}

}  // namespace fwd

// ------------------------------------------------------------------------------------
// dec_boost_kernel: one workgroup per logits row, threads stride over the table's target-id groups; the thread that owns
// a group matches its entries against the row's history (a uniform base pointer per row; a phrase is at most 32 compares)
// and does ONE add and ONE store for its id: no atomics, no order dependence.
// SCORE = false, the decode step: the history is the parity half of hist2 that *d_step selects, n = step, rows of done
// chunks return.  SCORE = true: row r is position pos0 + r % nb of sequence r / nb, as dec_score_kernel addresses it; a row
// without a target returns.
// ------------------------------------------------------------------------------------
#define BOOST_THREADS 256
template <bool SCORE>
__global__ __launch_bounds__(BOOST_THREADS) void dec_boost_kernel(float* __restrict__ logits, const int* __restrict__ boost_tab,
                                                                  int V, int K, int R, int NT, fwd::RowSource src) {
  const int r = blockIdx.x;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform)
  const fwd::BoostView tv = fwd::boost_view(boost_tab);
  float* lg = logits + (size_t)r * V;
  for (int g = threadIdx.x; g < tv.G; g += BOOST_THREADS) {
    float b;
    if (!fwd::boost_of_group(tv, tv.grp_off[g], tv.grp_off[g + 1], hist, n, b)) continue;
    const int v = tv.grp_id[g];
    if (v < V) lg[v] += b;   // (fw_boost_create checked the ids against the list's n_vocab, the callers that against V)
  }
}

namespace fwd {

void launch_boost_step(hipStream_t st, const GenDev& gp, float* logits, const int* boost_tab, const int* hist2,
                       const int* d_step, const int* done) {
  if (!boost_tab || gp.R <= 0) return;
  dec_boost_kernel<false><<<gp.R, BOOST_THREADS, 0, st>>>(logits, boost_tab, gp.V, gp.K, gp.R, gp.n_text_ctx,
                                                         {hist2, d_step, done, nullptr, 0, 0, 1});
}

void launch_boost_score(hipStream_t st, const GenDev& gp, float* logits, const int* boost_tab, const ScoreRow* tab,
                        int tab_stride, int pos0, int nb, int rows, const int* hist_pool) {
  if (!boost_tab || rows <= 0) return;
  dec_boost_kernel<true><<<rows, BOOST_THREADS, 0, st>>>(logits, boost_tab, gp.V, 1, rows, gp.n_text_ctx,
                                                        {hist_pool, nullptr, nullptr, tab, tab_stride, pos0, nb});
}

void boost_rows_host(const int* boost_tab, float* logits, int rows, int V, const int* hist, const int* hist_offsets) {
  const BoostView tv = boost_view(boost_tab);
  for (int r = 0; r < rows; ++r) {
    const int n = hist_offsets[r + 1] - hist_offsets[r];
    for (int g = 0; g < tv.G; ++g) {
      float b;
      if (!boost_of_group(tv, tv.grp_off[g], tv.grp_off[g + 1], hist + hist_offsets[r], n, b)) continue;
      if (tv.grp_id[g] < V) logits[(size_t)r * V + tv.grp_id[g]] += b;
    }
  }
}

int32_t phrase_list_check(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases, int max_phrases,
                          int max_len, int max_tokens) {
  FW_CHECK_ARG(n_vocab >= 1, "n_vocab %d must be positive", n_vocab);
  FW_CHECK_ARG(n_phrases >= 0 && n_phrases <= max_phrases, "%d phrases not in [0, %d]", n_phrases, max_phrases);
  if (n_phrases == 0) return FW_OK;
  FW_CHECK_ARG(tokens && offsets, "null argument");
  FW_CHECK_ARG(offsets[0] == 0, "offsets must start at 0");
  for (int j = 0; j < n_phrases; ++j) {
    // (compared as 64-bit values: offsets that decrease or jump cannot wrap the length)
    const int64_t len = (int64_t)offsets[j + 1] - offsets[j];
    FW_CHECK_ARG(len >= 1 && len <= max_len, "phrase %d has %lld tokens, not 1 .. %d", j, (long long)len, max_len);
    FW_CHECK_ARG(offsets[j + 1] <= max_tokens, "more than %d tokens in all", max_tokens);
  }
  for (int j = 0; j < n_phrases; ++j)
    for (int i = offsets[j]; i < offsets[j + 1]; ++i)
      FW_CHECK_ARG(tokens[i] >= 0 && tokens[i] < n_vocab, "phrase %d: token %d outside [0, %d)", j, tokens[i], n_vocab);
  return FW_OK;
}

}  // namespace fwd

extern "C" {

int32_t fw_boost_create(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
                        const float* boosts, fw_boost** out) {
  FW_CHECK_ARG(out, "null argument");
  *out = nullptr;
  if (int rc = fwd::phrase_list_check(n_vocab, tokens, offsets, n_phrases, FW_BOOST_MAX_PHRASES, FW_BOOST_MAX_LEN,
                                      FW_BOOST_MAX_TOKENS))
    return rc;
  FW_CHECK_ARG(n_phrases == 0 || boosts, "null argument");
  for (int j = 0; j < n_phrases; ++j) FW_CHECK_ARG(std::isfinite(boosts[j]), "the boost of phrase %d is not finite", j);
  const int T = n_phrases > 0 ? offsets[n_phrases] : 0;
  // entries (j, k) ordered by (target id, j, k): equal arguments give equal bytes
  struct Ent { int id, start, k, bits; };
  std::vector<Ent> ents;
  ents.reserve((size_t)T);
  for (int j = 0; j < n_phrases; ++j)
    for (int k = 0; k < offsets[j + 1] - offsets[j]; ++k) {
      int bits;
      memcpy(&bits, &boosts[j], sizeof(bits));
      ents.push_back({tokens[offsets[j] + k], offsets[j], k, bits});
    }
  std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.id < b.id; });
  std::vector<int32_t> grp_id, grp_off;
  for (int e = 0; e < T; ++e)
    if (e == 0 || ents[e].id != ents[e - 1].id) { grp_id.push_back(ents[e].id); grp_off.push_back(e); }
  grp_off.push_back(T);
  fw_boost* b = new (std::nothrow) fw_boost();
  if (!b) { fw::set_error("out of host memory"); return FW_ENOMEM; }
  b->n_vocab = n_vocab;
  std::vector<int32_t>& tab = b->table;
  tab.reserve((size_t)fwd::BOOST_HDR_WORDS + grp_id.size() + grp_off.size() + 4 * (size_t)T);
  tab.push_back((int32_t)grp_id.size()); tab.push_back(T); tab.push_back(T); tab.push_back(n_vocab);
  tab.insert(tab.end(), grp_id.begin(), grp_id.end());
  tab.insert(tab.end(), grp_off.begin(), grp_off.end());
  for (const Ent& e : ents) { tab.push_back(e.start); tab.push_back(e.k); tab.push_back(e.bits); }
  tab.insert(tab.end(), tokens, tokens + T);
  *out = b;
  return FW_OK;
}

void fw_boost_free(fw_boost* b) { delete b; }

}  // extern "C"
