// Shallow fusion with a back-off n-gram language model (include/fwamd.h: fw_ngram) for gfx950: the table compiler (host),
// dec_ngram_kernel — which adds scale * score(v) + bonus to every id v <= <eot> of a row of float32 logits, behind the
// boost and in front of the constraint / automaton and the rules kernel (decode steps) or the scoring kernel — and the
// same walk in plain C++.  The table layout (a dense unigram level, then a trie over reversed contexts): dec_kernels.h.
#include "engine.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <unordered_map>

#include "dec_kernels.h"

// ------------------------------------------------------------------------------------
// dec_ngram_kernel: one workgroup of four waves per logits row.  Unlike the mask writers (dec_constrain_kernel,
// dec_automaton_kernel) it READS the row: every id up to <eot> gets a value that depends on the row's last N - 1 text ids.
//   1. CONTEXT, by wave 0.  Only the last N - 1 text ids of the history matter: the wave ballots over the history from its
//      END backwards, 64 entries at a time, and takes the text ids (< ts_begin) in that order until it has N - 1 of them or
//      the history is used up — then BOS is the next symbol.  The symbols stay in scalar registers; nothing is compacted.
//   2. THE WALK, by wave 0, while waves 1 .. 3 clear the `done` bit mask (one bit per id up to <eot>) in LDS.  The trie is
//      over reversed contexts, so following the symbols in the order step 1 found them passes c_1, c_2, .. c_K: at most
//      N - 1 dependent transitions yield the whole back-off chain (LDS: chain[], the deepest level that has a record).
//      A transition is a 64-ARY SEARCH: the 64 lanes look at the last id of 64 equal slices of the node's child pairs, the
//      first slice whose last id is >= the symbol is the only one that can hold it; slices of at most 64 pairs are matched
//      with one coalesced 8-byte-per-lane fetch and a ballot.  The root of a large-v3 model has a child for most of its
//      51 866 ids: three fetches (64^3 > 2^17), where a scan in 64-pair chunks with 64 chunk ends per round took up to 14.
//   3. THE SPARSE LEVELS, from the longest context that has a record down to c_1, a workgroup barrier between two levels.
//      The threads stride over the node's successor pairs (id, p) — one 8-byte load each; the thread that wins the LDS
//      atomicOr test-and-set of the id's bit does the id's ONE read-add-write, with the back-offs accumulated above that
//      level.  Ids are unique within a node and the levels are barrier-separated: who writes an id, and what, does not
//      depend on timing.
//   4. THE DENSE PASS.  All threads stream logits[v] (16-byte loads and stores; up to three ids in front of the first
//      16-byte boundary of the row and up to three behind the last are peeled off, as fwd::write_neg_inf_row does) and
//      unigram[v] (four floats in one load at the alignment of a float: the table's alignment relative to the row's is
//      anybody's), and add to the ids whose bit is clear.  A group of four with no bit set takes one 16-byte store, a
//      mixed group one 4-byte store per clear bit, a group whose four ids the sparse levels served is not even loaded.
// Every id <= <eot> is written exactly once, the ids above it never; a -inf logit stays -inf (-inf + finite).
// SCORE = false / true: the two row forms of fwd::row_history, as the other pre-pass kernels have them.
// ------------------------------------------------------------------------------------
#define NGRAM_THREADS 256
// (one word more than the ids need: the 64-bit window of the dense pass's last group reads it)
#define NGRAM_MASK_WORDS (LP_SUP_WORDS * 2 + 1)

namespace fwd {

typedef float ngram_f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats, loaded at a float's alignment

// the record behind the child pair of record `rec` whose id is `t`, -1 without one.  Called by ONE whole wave; the result
// is wave-uniform.  Every 64-pair fetch stays inside the table by its padding.
static __device__ __forceinline__ int ngram_child(const int* __restrict__ tab, int rec, int t, int lane) {
  const int* pairs = tab + rec + NGRAM_REC_WORDS;
  int lo = 0, hi = __builtin_amdgcn_readfirstlane(tab[rec]);
  while (hi - lo > 64) {   // (uniform) 64 slices of `step` >= 2 pairs: the next range is one of them
    const int step = (hi - lo + 63) >> 6;
    const int first = lo + lane * step;
    const int last = min(first + step, hi) - 1;
    const unsigned long long b = __ballot(first < hi && pairs[2 * last] >= t);
    if (!b) return -1;   // t is above every id of the node
    lo += (__ffsll((long long)b) - 1) * step;
    hi = min(lo + step, hi);
  }
  const int2 e = *reinterpret_cast<const int2*>(pairs + 2 * (lo + lane));
  const unsigned long long hit = __ballot(lo + lane < hi && e.x == t);
  if (!hit) return -1;
  return __builtin_amdgcn_readlane(e.y, __ffsll((long long)hit) - 1);
}

}  // namespace fwd

template <bool SCORE>
__global__ __launch_bounds__(NGRAM_THREADS) void dec_ngram_kernel(float* __restrict__ logits, const int* __restrict__ tab,
                                                                  int V, int K, int R, int NT, int eot, int ts_begin,
                                                                  fwd::RowSource src) {
  __shared__ unsigned done[NGRAM_MASK_WORDS];
  __shared__ int chain[FW_NGRAM_MAX_ORDER - 1];
  __shared__ int chain_n;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform, in front of the first barrier)
  const int n_ids = eot + 1;

  if (wv == 0) {
    // 1. the context's symbols, the last one first
    const int want = min(tab[0], FW_NGRAM_MAX_ORDER) - 1;
    int sym[FW_NGRAM_MAX_ORDER - 1] = {0, 0, 0, 0};
    int n_sym = 0;
    const auto push = [&](int v) {
#pragma unroll
      for (int q = 0; q < FW_NGRAM_MAX_ORDER - 1; ++q) sym[q] = q == n_sym ? v : sym[q];
      ++n_sym;
    };
    for (int i0 = 0; i0 < n && n_sym < want; i0 += 64) {   // (uniform)
      const int i = n - 1 - i0 - lane;
      const int id = i >= 0 ? hist[i] : ts_begin;
      unsigned long long b = __ballot(id < ts_begin);
      while (b && n_sym < want) {
        push(__builtin_amdgcn_readlane(id, __ffsll((long long)b) - 1));
        b &= b - 1ull;
      }
    }
    if (n_sym < want) push(tab[2]);   // the whole history went by: BOS (= n_vocab) is in front of it
    // 2. the walk
    int rec = tab[7], depth = 0;
#pragma unroll
    for (int q = 0; q < FW_NGRAM_MAX_ORDER - 1; ++q) {
      if (q < n_sym && rec >= 0) {   // (uniform)
        rec = fwd::ngram_child(tab, rec, sym[q], lane);
        if (rec >= 0) {
          if (lane == 0) chain[q] = rec;
          depth = q + 1;
        }
      }
    }
    if (lane == 0) chain_n = depth;
  } else {
    const int n_words = (n_ids + 31) / 32 + 1;
    for (int w = tid - 64; w < n_words; w += NGRAM_THREADS - 64) done[w] = 0u;
  }
  __syncthreads();

  const float scale = fwd::ngram_bits_float(tab[4]), bonus = fwd::ngram_bits_float(tab[5]);
  float* lg = logits + (size_t)r * V;
  // 3. the sparse levels, the longest context first.  (the levels between it and c_K have no record: back-off 0, and
  //    0.0f + 0.0f is the 0.0f the accumulator starts with)
  float acc = 0.0f;
  for (int k = chain_n; k >= 1; --k) {   // (uniform)
    const int rec = chain[k - 1];
    const int n_succ = tab[rec + 1];
    const int* succ = tab + rec + fwd::NGRAM_REC_WORDS + 2 * tab[rec];
    for (int i = tid; i < n_succ; i += NGRAM_THREADS) {
      const int2 e = *reinterpret_cast<const int2*>(succ + 2 * i);
      if ((unsigned)e.x >= (unsigned)n_ids) continue;   // (the callers refuse such a table: never outside the row anyway)
      const unsigned bit = 1u << (e.x & 31);
      if (!(atomicOr(&done[e.x >> 5], bit) & bit)) lg[e.x] += scale * (acc + fwd::ngram_bits_float(e.y)) + bonus;
    }
    acc += fwd::ngram_bits_float(tab[rec + 2]);
    __syncthreads();
  }

  // 4. the dense pass: the unigram level under every back-off of the chain
  const float* uni = reinterpret_cast<const float*>(tab + fwd::NGRAM_HDR_WORDS);
  const auto is_done = [&](int v) { return (done[v >> 5] >> (v & 31)) & 1u; };
  int head = (int)(((16u - (unsigned)((uintptr_t)lg & 15u)) & 15u) >> 2);   // ids in front of the first 16-byte boundary
  head = head < n_ids ? head : n_ids;
  const int n_vec = (n_ids - head) >> 2, tail0 = head + 4 * n_vec;
  if (tid < head && !is_done(tid)) lg[tid] += scale * (acc + uni[tid]) + bonus;
  {
    const int v = tail0 + tid;   // tid < 3 at most
    if (v < n_ids && !is_done(v)) lg[v] += scale * (acc + uni[v]) + bonus;
  }
  for (int i = tid; i < n_vec; i += NGRAM_THREADS) {
    const int v0 = head + 4 * i;   // v0 + 3 < tail0 <= n_ids
    const int w = v0 >> 5;
    const unsigned long long win = ((unsigned long long)done[w + 1] << 32) | done[w];
    const unsigned d4 = (unsigned)(win >> (v0 & 31)) & 15u;
    if (d4 == 15u) continue;
    float4 x = *reinterpret_cast<const float4*>(lg + v0);
    const fwd::ngram_f4u u = *reinterpret_cast<const fwd::ngram_f4u*>(uni + v0);
    x.x += scale * (acc + u.x) + bonus;
    x.y += scale * (acc + u.y) + bonus;
    x.z += scale * (acc + u.z) + bonus;
    x.w += scale * (acc + u.w) + bonus;
    if (d4 == 0u) {
      *reinterpret_cast<float4*>(lg + v0) = x;
    } else {
      if (!(d4 & 1u)) lg[v0] = x.x;
      if (!(d4 & 2u)) lg[v0 + 1] = x.y;
      if (!(d4 & 4u)) lg[v0 + 2] = x.z;
      if (!(d4 & 8u)) lg[v0 + 3] = x.w;
    }
  }
}

namespace fwd {

// what the kernel's bit mask holds
static bool ngram_gp_ok(int V, int eot, int ts_begin) {
  return V >= 1 && V <= LP_SUP_WORDS * 64 && eot >= 0 && eot < ts_begin && ts_begin <= V;
}

bool ngram_geometry_ok(const int* tab, int V, int eot, int ts_begin) {
  return ngram_gp_ok(V, eot, ts_begin) && tab[2] == V && tab[3] == eot && tab[6] <= eot;
}

void launch_ngram(hipStream_t st, const GenDev& gp, float* logits, const int* tab, const RowSource& src, int rows) {
  const bool step = src.tab == nullptr;
  if (!tab || (step ? gp.R : rows) <= 0 || !ngram_gp_ok(gp.V, gp.eot, gp.ts_begin)) return;
  if (step)
    dec_ngram_kernel<false><<<gp.R, NGRAM_THREADS, 0, st>>>(logits, tab, gp.V, gp.K, gp.R, gp.n_text_ctx, gp.eot, gp.ts_begin, src);
  else
    dec_ngram_kernel<true><<<rows, NGRAM_THREADS, 0, st>>>(logits, tab, gp.V, 1, rows, gp.n_text_ctx, gp.eot, gp.ts_begin, src);
}

// one transition in plain C++: a binary search over the node's child pairs
static int ngram_child_host(const int* tab, int rec, int t) {
  const int* pairs = tab + rec + NGRAM_REC_WORDS;
  int lo = 0, hi = tab[rec];
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (pairs[2 * mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo < tab[rec] && pairs[2 * lo] == t ? pairs[2 * lo + 1] : -1;
}

void ngram_rows_host(const int* tab, float* logits, int rows, int V, int eot, int ts_begin, const int* hist,
                     const int* hist_offsets) {
  if (!ngram_geometry_ok(tab, V, eot, ts_begin)) return;
  const int want = tab[0] - 1;
  const float scale = ngram_bits_float(tab[4]), bonus = ngram_bits_float(tab[5]);
  const float* uni = reinterpret_cast<const float*>(tab + NGRAM_HDR_WORDS);
  std::vector<char> done((size_t)eot + 1);
  for (int r = 0; r < rows; ++r) {
    int chain[FW_NGRAM_MAX_ORDER - 1], depth = 0, n_sym = 0, rec = tab[7];
    for (int i = hist_offsets[r + 1] - 1; i >= hist_offsets[r] - 1 && n_sym < want && rec >= 0; --i) {
      if (i >= hist_offsets[r] && hist[i] >= ts_begin) continue;
      rec = ngram_child_host(tab, rec, i >= hist_offsets[r] ? hist[i] : tab[2]);   // (one step past the start: BOS)
      ++n_sym;
      if (rec >= 0) chain[depth++] = rec;
    }
    std::fill(done.begin(), done.end(), 0);
    float* lg = logits + (size_t)r * V;
    float acc = 0.0f;
    for (int k = depth; k >= 1; --k) {
      const int nd = chain[k - 1];
      const int* succ = tab + nd + NGRAM_REC_WORDS + 2 * tab[nd];
      for (int i = 0; i < tab[nd + 1]; ++i) {
        const int v = succ[2 * i];
        if (v < 0 || v > eot || done[v]) continue;
        done[v] = 1;
        lg[v] += scale * (acc + ngram_bits_float(succ[2 * i + 1])) + bonus;
      }
      acc += ngram_bits_float(tab[nd + 2]);
    }
    for (int v = 0; v <= eot; ++v)
      if (!done[v]) lg[v] += scale * (acc + uni[v]) + bonus;
  }
}

}  // namespace fwd

extern "C" {

int32_t fw_ngram_create(int32_t n_vocab, int32_t order, const int32_t* counts, const int32_t* ids, const float* logprobs,
                        const float* backoffs, float unk_logprob, float scale, float bonus, int32_t eos_id, fw_ngram** out) {
  FW_CHECK_ARG(out, "null argument");
  *out = nullptr;
  FW_CHECK_ARG(n_vocab >= 1, "n_vocab %d must be positive", n_vocab);
  FW_CHECK_ARG(order >= 1 && order <= FW_NGRAM_MAX_ORDER, "order %d not in [1, %d]", order, FW_NGRAM_MAX_ORDER);
  FW_CHECK_ARG(counts, "null argument: counts");
  FW_CHECK_ARG(eos_id >= 0 && eos_id < n_vocab, "eos_id %d outside [0, %d)", eos_id, n_vocab);
  FW_CHECK_ARG(std::isfinite(unk_logprob) && std::isfinite(scale) && std::isfinite(bonus),
               "unk_logprob %g, scale %g and bonus %g must be finite", (double)unk_logprob, (double)scale, (double)bonus);
  int64_t n_high = 0, n_all = 0, n_with_bo = 0;
  for (int k = 1; k <= order; ++k) {
    FW_CHECK_ARG(counts[k - 1] >= 0, "order %d: a count of %d n-grams", k, counts[k - 1]);
    n_all += counts[k - 1];
    if (k >= 2) n_high += counts[k - 1];
    if (k < order) n_with_bo += counts[k - 1];
  }
  FW_CHECK_ARG(n_high <= FW_NGRAM_MAX_GRAMS, "%lld n-grams of order 2 and above, more than %d", (long long)n_high, FW_NGRAM_MAX_GRAMS);
  FW_CHECK_ARG(n_all == 0 || (ids && logprobs), "null argument: ids / logprobs with %lld n-grams", (long long)n_all);
  FW_CHECK_ARG(n_with_bo == 0 || backoffs, "null argument: backoffs with %lld n-grams below order %d", (long long)n_with_bo, order);
  const int BOS = n_vocab;
  try {
    // the trie's nodes in the order the n-grams first need them (node 0: the root), their children and successors as lists
    std::vector<float> node_bo(1, 0.0f);
    std::unordered_map<uint64_t, int> child_of;   // (parent node << 32 | id) -> node
    struct Child { int parent, id, node; };
    struct Succ { int node, id; float p; int order, index; };
    std::vector<Child> children;
    std::vector<Succ> succs;
    const auto node_for = [&](const int32_t* w, int k) {   // the node of context w[0 .. k): along w[k - 1], .. w[0]
      int nd = 0;
      for (int j = k - 1; j >= 0; --j) {
        const uint64_t key = ((uint64_t)nd << 32) | (uint32_t)w[j];
        const auto it = child_of.find(key);
        if (it != child_of.end()) { nd = it->second; continue; }
        const int nn = (int)node_bo.size();
        node_bo.push_back(0.0f);
        child_of.emplace(key, nn);
        children.push_back({nd, w[j], nn});
        nd = nn;
      }
      return nd;
    };
    std::vector<float> uni((size_t)fwd::ngram_unigram_words(eos_id), 0.0f);
    std::fill(uni.begin(), uni.begin() + eos_id + 1, unk_logprob);
    std::vector<char> uni_seen((size_t)n_vocab + 1, 0);
    int max_id = -1;
    size_t at_id = 0, at = 0;   // into ids, into logprobs / backoffs
    for (int k = 1; k <= order; ++k)
      for (int g = 0; g < counts[k - 1]; ++g, at_id += k, ++at) {
        const int32_t* w = ids + at_id;
        const float p = logprobs[at], bo = k < order ? backoffs[at] : 0.0f;
        for (int j = 0; j < k; ++j) {
          FW_CHECK_ARG(w[j] >= 0 && w[j] <= n_vocab, "order %d, n-gram %d: id %d outside [0, %d]", k, g, w[j], n_vocab);
          FW_CHECK_ARG(w[j] != BOS || j == 0, "order %d, n-gram %d: BOS (%d) at position %d, it may only be the first id", k, g,
                       BOS, j);
          FW_CHECK_ARG(w[j] != eos_id || j == k - 1, "order %d, n-gram %d: eos_id %d inside the context (position %d)", k, g,
                       eos_id, j);
          if (w[j] != BOS) max_id = std::max(max_id, w[j]);
        }
        FW_CHECK_ARG(std::isfinite(p) && std::isfinite(bo), "order %d, n-gram %d: log-prob %g / back-off %g is not finite", k, g,
                     (double)p, (double)bo);
        const int v = w[k - 1];
        if (k == 1) {
          FW_CHECK_ARG(!uni_seen[v], "order 1, n-gram %d: id %d has a unigram already (a duplicate)", g, v);
          uni_seen[v] = 1;
          FW_CHECK_ARG(v != BOS || p == 0.0f, "order 1, n-gram %d: BOS with log-prob %g — BOS is never predicted, its unigram "
                       "carries a back-off weight only (log-prob 0)", g, (double)p);
          if (v <= eos_id) uni[v] = p;
        } else {
          succs.push_back({node_for(w, k - 1), v, p, k, g});
        }
        // (a back-off of 0 needs no record — that is what a missing one means — and no history holds eos_id)
        if (bo != 0.0f && v != eos_id) node_bo[node_for(w, k)] = bo;
      }
    std::sort(children.begin(), children.end(),
              [](const Child& a, const Child& b) { return a.parent != b.parent ? a.parent < b.parent : a.id < b.id; });
    std::sort(succs.begin(), succs.end(), [](const Succ& a, const Succ& b) {
      return a.node != b.node ? a.node < b.node : a.id != b.id ? a.id < b.id : a.order != b.order ? a.order < b.order : a.index < b.index;
    });
    for (size_t i = 1; i < succs.size(); ++i)
      FW_CHECK_ARG(succs[i].node != succs[i - 1].node || succs[i].id != succs[i - 1].id,
                   "order %d, n-gram %d: a duplicate of n-gram %d", succs[i].order, succs[i].index, succs[i - 1].index);
    // record offsets: the nodes in creation order
    const size_t n_nodes = node_bo.size();
    std::vector<int32_t> n_child(n_nodes, 0), n_succ(n_nodes, 0), rec(n_nodes);
    for (const Child& c : children) ++n_child[c.parent];
    for (const Succ& s : succs) ++n_succ[s.node];
    int64_t words = fwd::NGRAM_HDR_WORDS + (int64_t)uni.size();
    for (size_t i = 0; i < n_nodes; ++i) {
      rec[i] = (int32_t)words;
      words += fwd::NGRAM_REC_WORDS + 2 * ((int64_t)n_child[i] + n_succ[i]);
      FW_CHECK_ARG(words < INT32_MAX - 1024, "the model compiles to more than 2^31 table words");
    }
    words = (words + fwd::NGRAM_PAD_WORDS + 3) & ~(int64_t)3;
    fw_ngram* lm = new (std::nothrow) fw_ngram();
    if (!lm) { fw::set_error("out of host memory"); return FW_ENOMEM; }
    std::unique_ptr<fw_ngram> hold(lm);
    lm->n_vocab = n_vocab;
    std::vector<int32_t>& tab = lm->table;
    tab.assign((size_t)words, -1);
    const auto bits = [](float f) { int32_t i; memcpy(&i, &f, 4); return i; };
    const int32_t hdr[fwd::NGRAM_HDR_WORDS] = {order, (int32_t)n_nodes, n_vocab, eos_id, bits(scale), bits(bonus), max_id, rec[0]};
    std::copy(hdr, hdr + fwd::NGRAM_HDR_WORDS, tab.begin());
    for (size_t i = 0; i < uni.size(); ++i) tab[fwd::NGRAM_HDR_WORDS + i] = bits(uni[i]);
    std::vector<int32_t> fill_c(n_nodes), fill_s(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
      int32_t* r = &tab[rec[i]];
      r[0] = n_child[i]; r[1] = n_succ[i]; r[2] = bits(node_bo[i]); r[3] = 0;
      fill_c[i] = rec[i] + fwd::NGRAM_REC_WORDS;
      fill_s[i] = fill_c[i] + 2 * n_child[i];
    }
    for (const Child& c : children) { tab[fill_c[c.parent]++] = c.id; tab[fill_c[c.parent]++] = rec[c.node]; }
    for (const Succ& s : succs) { tab[fill_s[s.node]++] = s.id; tab[fill_s[s.node]++] = bits(s.p); }
    *out = hold.release();
  } catch (const std::bad_alloc&) {
    fw::set_error("out of host memory");
    return FW_ENOMEM;
  }
  return FW_OK;
}

void fw_ngram_free(fw_ngram* lm) { delete lm; }

}  // extern "C"
