// Phrase boosting at catalogue scale (include/fwamd.h: fw_boost_create_large) for gfx950: the trie compiler (host),
// dec_boost_trie_kernel — which adds the boosts of a list of up to 65 536 phrases to a row of float32 logits, in
// dec_boost_kernel's place and with its bits — and the same walk in plain C++.  The table layout (one record per
// phrase prefix that some phrase continues): dec_kernels.h.
//
// What the definition becomes on a trie.  A node is a phrase prefix; the edge u -> v carries the largest boost of the
// phrases through it.  The pair (j, k) matches a row exactly when the node p_j[0 .. k) is a suffix of the row's history, so
// the row's candidates are the edges of the MATCHED nodes: the root and at most 31 more, one per suffix length, all found
// from the last 31 ids.  The boost of an id is the maximum over the matched nodes that have an edge with it.
//
// How the matched nodes are found: INDEPENDENT SUFFIX WALKS, not a goto / fail automaton.  Suffix length k is matched by
// walking h[n - k .. n) down from the root; the 31 walks share nothing, so the table needs no failure links (it stays a
// pure function of the phrase set, half the size, and the host compiler stays a sort and a scan), and a decode step — which
// sees a row's history afresh every launch, with no state carried from the step before — gains nothing from the amortised
// bound that failure links buy a streaming matcher: it would have to replay up to 31 dependent transitions per row anyway.
// Here the first transition of all 31 walks is ONE lane-parallel look-up in the root, almost every walk ends there (a
// history position rarely starts a listed phrase), and the few survivors are spread over the four waves.
//
// The root level is SPARSE: the root's (id, boost) pairs are strided over like any node's, one 8-byte load and one
// scattered 4-byte read-add-write per edge, and the 31 first transitions are binary searches of its pairs.  The alternative —
// a float and a child offset per id up to the largest first token, streamed beside the row in 16-byte groups as the n-gram
// kernel streams its unigram level — was built and measured against it on an MI355X (51 866 ids, 80 and 640 rows): with
// 9 700, 18 800 and 31 700 distinct first tokens below id 40 000 the two were within 7 % of each other either way (44.3 /
// 44.4 us at 31 700 and 80 rows), and with 1 014 and 16 the dense level cost its pass over the ids whatever the list held
// (28.5 against 4.5 us, 10.6 against 2.6).  It never won by more than the spread of a repeated run, so it is not kept:
// the cost is per root EDGE, and a short list pays nothing for the vocabulary.
#include "engine.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "dec_kernels.h"

namespace fwd {

// the index of the pair with id `t` among `n` pairs ascending by id, -1 without one
static __host__ __device__ __forceinline__ int boost_trie_find(const int* pairs, int n, int t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pairs[2 * mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo < n && pairs[2 * lo] == t ? lo : -1;
}

// one transition: the record behind the edge of record `rec` with id `t`; 0 without such an edge, or when nothing
// continues behind it
static __host__ __device__ __forceinline__ int boost_trie_child(const int* tab, int rec, int t) {
  const int* pairs = tab + rec + BOOST_TRIE_REC_WORDS;
  const int i = boost_trie_find(pairs, tab[rec], t);
  return i < 0 ? 0 : pairs[2 * i + 1];
}

// THE rule of who adds what, called per candidate edge by the kernel's two row forms and by the host walk.  list[0 .. M)
// are the records of the row's matched nodes, the root first, then by depth; the candidate is the edge (v, b) of list[i].
// False: a deeper matched node has an edge with v too, and that edge's owner adds.  True: this edge's owner adds `out`, the
// fp32 maximum of b and of the boosts the shallower matched nodes hold for v.  So every id with a candidate is added to
// exactly once, whoever runs first.
static __host__ __device__ __forceinline__ bool boost_trie_edge_value(const int* tab, const int* list, int M, int i, int v,
                                                                      float b, float& out) {
  for (int j = i + 1; j < M; ++j) {
    const int rec = list[j], cnt = tab[rec];
    if (boost_trie_find(tab + rec + BOOST_TRIE_REC_WORDS + 2 * cnt, cnt, v) >= 0) return false;
  }
  for (int j = 0; j < i; ++j) {
    const int rec = list[j], cnt = tab[rec];
    const int* bp = tab + rec + BOOST_TRIE_REC_WORDS + 2 * cnt;
    const int at = boost_trie_find(bp, cnt, v);
    if (at < 0) continue;
    const float o = ngram_bits_float(bp[2 * at + 1]);
    b = o > b ? o : b;   // (fp32 max over finite values)
  }
  out = b;
  return true;
}

// boost_trie_child by ONE whole wave, as a 64-ary search (dec_ngram.hip has the reasoning): the result is wave-uniform,
// and every 64-pair fetch stays inside the table by its padding.
static __device__ __forceinline__ int boost_trie_child_wave(const int* __restrict__ tab, int rec, int t, int lane) {
  const int* pairs = tab + rec + BOOST_TRIE_REC_WORDS;
  int lo = 0, hi = __builtin_amdgcn_readfirstlane(tab[rec]);
  while (hi - lo > 64) {   // (uniform) 64 slices of `step` >= 2 pairs: the next range is one of them
    const int step = (hi - lo + 63) >> 6;
    const int first = lo + lane * step;
    const int last = min(first + step, hi) - 1;
    const unsigned long long b = __ballot(first < hi && pairs[2 * last] >= t);
    if (!b) return 0;   // t is above every id of the node
    lo += (__ffsll((long long)b) - 1) * step;
    hi = min(lo + step, hi);
  }
  const int2 e = *reinterpret_cast<const int2*>(pairs + 2 * (lo + lane));
  const unsigned long long hit = __ballot(lo + lane < hi && e.x == t);
  if (!hit) return 0;
  return __builtin_amdgcn_readlane(e.y, __ffsll((long long)hit) - 1);
}

}  // namespace fwd

// ------------------------------------------------------------------------------------
// dec_boost_trie_kernel: one workgroup of four waves per logits row.
//   1. FIRST TRANSITIONS.  Thread k, 1 <= k <= min(n, 31), looks h[n - k] up in the root: a binary search of its pairs.
//      Nothing in front of h[0] is read: k <= n.
//   2. THE WALKS.  Every wave sees the same surviving suffix lengths (a ballot over step 1's results in LDS) and takes
//      every fourth of them: k - 1 more dependent transitions along h[n - k + 1 .. n), each a wave-wide search.  A walk
//      that reaches a node with edges leaves its record in LDS.  Wave 0 then compacts them behind the root, by depth.
//   3. THE NODES.  Matched node after matched node, the root first, the threads stride over the node's
//      (id, boost) pairs — one 8-byte load each — and fwd::boost_trie_edge_value says whether this edge's thread adds, and
//      what.  One read-add-write of 4 bytes per id; no atomics on the row, no barrier between the nodes: two threads never
//      own one id.  The rule searches the other matched nodes, a chain of dependent loads per edge; the ROOT's edges — tens
//      of thousands — are spared it by a filter: when a row has deeper matched nodes, the ids on their edges are hashed
//      into 8 192 bits of LDS first, and a root edge whose bit is clear (nearly all) is on no deeper node and is added as
//      it stands.  A set bit only means that the rule is asked.
// LDS: 1 412 bytes.  No id >= V is touched: a pair with a larger id is passed over.
// SCORE = false / true: the two row forms of fwd::row_history, as the other pre-pass kernels have them.
// ------------------------------------------------------------------------------------
#define BTRIE_THREADS 256
template <bool SCORE>
__global__ __launch_bounds__(BTRIE_THREADS) void dec_boost_trie_kernel(float* __restrict__ logits, const int* __restrict__ tab,
                                                                       int V, int K, int R, int NT, fwd::RowSource src) {
  __shared__ int s_start[32];   // [k]: where h[n - k] leads from the root (0: nowhere)
  __shared__ int s_node[32];    // [k]: the record of the node that equals the history's last k ids (0: none with edges)
  __shared__ int s_list[32];    // the matched nodes with edges, the root first, then by depth
  __shared__ int s_M;
  __shared__ unsigned s_maybe[BTRIE_THREADS];   // bit (v mod 8192): some deeper matched node may have an edge with v
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform, in front of the first barrier)
  const int root = tab[4];
  const int kmax = min(n, fwd::BOOST_TRIE_MAX_DEPTH);

  // 1. the first transition of every suffix length
  if (tid < 32) {
    int c = 0;
    if (tid >= 1 && tid <= kmax) c = fwd::boost_trie_child(tab, root, hist[n - tid]);
    s_start[tid] = c;
    s_node[tid] = tid == 1 ? c : 0;
  }
  __syncthreads();

  // 2. the walks that go on, every fourth one to this wave
  {
    const int c = lane < 32 ? s_start[lane] : 0;
    int rank = 0;
    for (unsigned long long b = __ballot(lane >= 2 && c != 0); b; b &= b - 1ull, ++rank) {   // (uniform)
      if ((rank & 3) != wv) continue;
      const int k = __ffsll((long long)b) - 1;
      int rec = __builtin_amdgcn_readlane(c, k);
      for (int q = 1; q < k && rec; ++q) rec = fwd::boost_trie_child_wave(tab, rec, hist[n - k + q], lane);
      if (lane == 0) s_node[k] = rec;
    }
  }
  __syncthreads();
  if (wv == 0) {
    const int nd = (lane >= 1 && lane < 32) ? s_node[lane] : 0;
    const unsigned long long b = __ballot(nd != 0);
    if (nd) s_list[1 + __popcll(b & ((1ull << lane) - 1ull))] = nd;
    if (lane == 0) { s_list[0] = root; s_M = 1 + __popcll(b); }
  }
  __syncthreads();

  const int M = s_M;
  if (M > 1) {   // (uniform) the filter over the deeper nodes' ids
    s_maybe[tid] = 0u;
    __syncthreads();
    for (int i = 1; i < M; ++i) {
      const int rec = s_list[i], cnt = tab[rec];
      const int* bp = tab + rec + fwd::BOOST_TRIE_REC_WORDS + 2 * cnt;
      for (int e = tid; e < cnt; e += BTRIE_THREADS) {
        const int v = bp[2 * e];
        atomicOr(&s_maybe[(v >> 5) & (BTRIE_THREADS - 1)], 1u << (v & 31));
      }
    }
    __syncthreads();
  }
  const auto maybe = [&](int v) { return M > 1 && ((s_maybe[(v >> 5) & (BTRIE_THREADS - 1)] >> (v & 31)) & 1u) != 0u; };

  // 3. the matched nodes
  float* lg = logits + (size_t)r * V;
  for (int i = 0; i < M; ++i) {   // (uniform)
    const int rec = s_list[i], cnt = tab[rec];
    const int* bp = tab + rec + fwd::BOOST_TRIE_REC_WORDS + 2 * cnt;
    for (int e = tid; e < cnt; e += BTRIE_THREADS) {
      const int2 p = *reinterpret_cast<const int2*>(bp + 2 * e);
      if ((unsigned)p.x >= (unsigned)V) continue;   // (the callers refuse such a list: never outside the row anyway)
      float b = fwd::ngram_bits_float(p.y);
      if ((i > 0 || maybe(p.x)) && !fwd::boost_trie_edge_value(tab, s_list, M, i, p.x, b, b)) continue;
      lg[p.x] += b;
    }
  }
}

namespace fwd {

void launch_boost_trie(hipStream_t st, const GenDev& gp, float* logits, const int* tab, const RowSource& src, int rows) {
  const bool step = src.tab == nullptr;
  if (!tab || (step ? gp.R : rows) <= 0) return;
  if (step)
    dec_boost_trie_kernel<false><<<gp.R, BTRIE_THREADS, 0, st>>>(logits, tab, gp.V, gp.K, gp.R, gp.n_text_ctx, src);
  else
    dec_boost_trie_kernel<true><<<rows, BTRIE_THREADS, 0, st>>>(logits, tab, gp.V, 1, rows, gp.n_text_ctx, src);
}

void boost_trie_rows_host(const int* tab, float* logits, int rows, int V, const int* hist, const int* hist_offsets) {
  for (int r = 0; r < rows; ++r) {
    const int* h = hist + hist_offsets[r];
    const int n = hist_offsets[r + 1] - hist_offsets[r];
    int list[BOOST_TRIE_MAX_DEPTH + 1], M = 1;
    list[0] = tab[4];
    for (int k = 1; k <= std::min(n, BOOST_TRIE_MAX_DEPTH); ++k) {
      int rec = tab[4];
      for (int q = 0; q < k && rec; ++q) rec = boost_trie_child(tab, rec, h[n - k + q]);
      if (rec) list[M++] = rec;
    }
    for (int i = 0; i < M; ++i) {
      const int cnt = tab[list[i]];
      const int* bp = tab + list[i] + BOOST_TRIE_REC_WORDS + 2 * cnt;
      for (int e = 0; e < cnt; ++e) {
        float b;
        if (bp[2 * e] < V && boost_trie_edge_value(tab, list, M, i, bp[2 * e], ngram_bits_float(bp[2 * e + 1]), b))
          logits[(size_t)r * V + bp[2 * e]] += b;
      }
    }
  }
}

}  // namespace fwd

extern "C" int32_t fw_boost_create_large(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
                                         const float* boosts, fw_boost** out) {
  using namespace fwd;
  FW_CHECK_ARG(out, "null argument");
  *out = nullptr;
  if (int rc = phrase_list_check(n_vocab, tokens, offsets, n_phrases, FW_BOOST_LARGE_MAX_PHRASES, FW_BOOST_MAX_LEN,
                                 FW_BOOST_LARGE_MAX_TOKENS))
    return rc;
  FW_CHECK_ARG(n_phrases == 0 || boosts, "null argument");
  for (int j = 0; j < n_phrases; ++j) FW_CHECK_ARG(std::isfinite(boosts[j]), "the boost of phrase %d is not finite", j);
  try {
    // the phrases by their ids, lexicographically: the nodes below are then numbered in the trie's pre-order, and the
    // children of a node appear by ascending id — whatever order and however often the caller named the phrases
    std::vector<int> order((size_t)n_phrases);
    for (int j = 0; j < n_phrases; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      return std::lexicographical_compare(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b], tokens + offsets[b + 1]);
    });
    std::vector<int32_t> parent(1, -1), id(1, -1), n_child(1, 0);
    std::vector<float> best(1, 0.0f);   // of node v: the largest boost through the edge that enters v
    int path[FW_BOOST_MAX_LEN + 1] = {0}, prev = -1;
    for (int j : order) {
      const int32_t* p = tokens + offsets[j];
      const int L = offsets[j + 1] - offsets[j];
      int lcp = 0;
      if (prev >= 0) {
        const int32_t* q = tokens + offsets[prev];
        const int Lq = offsets[prev + 1] - offsets[prev];
        while (lcp < L && lcp < Lq && p[lcp] == q[lcp]) ++lcp;
      }
      // (the larger one, and +0 over -0: what an edge holds does not depend on the order of the phrases)
      for (int d = 0; d < lcp; ++d) {
        float& m = best[path[d + 1]];
        if (boosts[j] > m || (boosts[j] == m && !std::signbit(boosts[j]))) m = boosts[j];
      }
      for (int d = lcp; d < L; ++d) {
        const int nn = (int)parent.size();
        parent.push_back(path[d]); id.push_back(p[d]); n_child.push_back(0); best.push_back(boosts[j]);
        ++n_child[path[d]];
        path[d + 1] = nn;
      }
      prev = j;
    }
    const size_t n_nodes = parent.size();
    std::vector<int32_t> rec(n_nodes, 0);
    int64_t words = BOOST_TRIE_HDR_WORDS;
    int n_rec = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
      if (i && !n_child[i]) continue;   // (nothing continues behind it: no record, its parent's pair holds 0)
      rec[i] = (int32_t)words;
      words += BOOST_TRIE_REC_WORDS + 4 * (int64_t)n_child[i];
      ++n_rec;
    }
    words = (words + BOOST_TRIE_PAD_WORDS + 3) & ~(int64_t)3;
    fw_boost* b = new (std::nothrow) fw_boost();
    if (!b) { fw::set_error("out of host memory"); return FW_ENOMEM; }
    std::unique_ptr<fw_boost> hold(b);
    b->n_vocab = n_vocab;
    b->large = true;
    std::vector<int32_t>& tab = b->table;
    tab.assign((size_t)words, -1);
    const auto bits = [](float f) { int32_t i; memcpy(&i, &f, 4); return i; };
    const int32_t hdr[BOOST_TRIE_HDR_WORDS] = {(int32_t)n_nodes - 1, n_rec, n_vocab, BOOST_TRIE_FORM_MARK, rec[0], 0, 0, 0};
    std::copy(hdr, hdr + BOOST_TRIE_HDR_WORDS, tab.begin());
    std::vector<int32_t> fill(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
      if (!rec[i]) continue;
      tab[rec[i]] = n_child[i]; tab[rec[i] + 1] = 0;
      fill[i] = rec[i] + BOOST_TRIE_REC_WORDS;
    }
    for (size_t v = 1; v < n_nodes; ++v) {   // (a node's children are created by ascending id)
      const int u = parent[v];
      int32_t& at = fill[u];
      tab[at] = id[v]; tab[at + 1] = rec[v];
      tab[at + 2 * n_child[u]] = id[v]; tab[at + 2 * n_child[u] + 1] = bits(best[v]);
      at += 2;
    }
    *out = hold.release();
  } catch (const std::bad_alloc&) {
    fw::set_error("out of host memory");
    return FW_ENOMEM;
  }
  return FW_OK;
}

