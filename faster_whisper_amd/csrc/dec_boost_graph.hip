// Revocable phrase boosting (include/fwamd.h: fw_boost_create_revocable) for gfx950: the context-graph compiler (host),
// dec_boost_graph_kernel — which gives every id up to <eot> of a row of float32 logits the bonus its token would earn,
// bank or lose on an Aho-Corasick automaton over the listed phrases — and the same walk in plain C++.  The table layout
// (one record per phrase prefix, with its failure link): dec_kernels.h.
//
// What differs from the sticky forms (dec_boost.hip, dec_boost_trie.hip).  Those add the boost of every edge of EVERY node
// that equals a suffix of the history, and never subtract.  Here a row has ONE state s, the deepest such node, which holds
// the bonus G(s) of the partial match; a token either extends a match (from s, or from the deepest node of s's failure
// chain that can take it) and is paid val(target) - G(s), or breaks it and is charged -G(s).  The second case is every
// id of the row that is on no edge of the chain: a dense pass the sticky forms do not have, and the reason this kernel
// holds a claim mask — one bit per id — between its sparse and its dense pass, as dec_ngram_kernel does.
//
// The state is found WITHOUT failure hops: no state is carried between steps, so a step would have to replay the history
// through the automaton — up to 32 dependent transitions, each with a chain of failure hops whose length depends on the
// list.  Instead 32 lanes walk the 32 suffix lengths of the row's last 32 text ids down from the root independently, and
// the deepest walk that arrives is s by definition: at most 32 x 32 child searches whatever the history and the list.
// The failure links are only FOLLOWED, from s to the root, to find who claims an id.
#include "engine.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "dec_kernels.h"

namespace fwd {

// one transition: the second word of the child pair of record `rec` whose id is `t` (the child's record), 0 without one
static __host__ __device__ __forceinline__ int boost_graph_child(const int* tab, int rec, int t) {
  const int* pairs = tab + rec + BOOST_GRAPH_REC_WORDS;
  int lo = 0, hi = tab[rec];
  const int n = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pairs[2 * mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo < n && pairs[2 * lo] == t ? pairs[2 * lo + 1] : 0;
}

// the node whose string is the row's last k text ids (tl[j]: the j-th last one), 0 when there is none: one of the 32
// independent walks, the kernel's lane k - 1 and the host walk's iteration k
static __host__ __device__ __forceinline__ int boost_graph_suffix_node(const int* tab, const int* tl, int k) {
  int rec = tab[4];
  for (int q = k - 1; q >= 0 && rec; --q) rec = boost_graph_child(tab, rec, tl[q]);
  return rec;
}

// what an id is given whose token leads to a node of value `val_bits` from a state that holds G: ONE fp32 subtract (the
// add to the logit is the caller's).  An id that continues nothing leads to the root, whose value is 0.
static __host__ __device__ __forceinline__ float boost_graph_delta(int val_bits, float G) { return ngram_bits_float(val_bits) - G; }

}  // namespace fwd

// ------------------------------------------------------------------------------------
// dec_boost_graph_kernel: one workgroup of four waves per logits row, four phases between workgroup barriers.
//   1. GATHER, by wave 0, while waves 1 .. 3 clear the claim mask (one bit per id up to <eot>) in LDS.  The wave ballots
//      over the history from its END backwards, 64 entries at a time, and puts the text ids (< ts_begin) into LDS in that
//      order until it has 32 of them or the history is used up: a phrase holds at most 32 tokens.
//   2. STATE, by the first 32 lanes of wave 0.  Lane k - 1 walks the last k text ids down from the root
//      (fwd::boost_graph_suffix_node: binary searches, no failure hops); the highest lane that arrives holds s.
//   3. THE SPARSE PASS over the chain s, fail(s), .. root, deepest first, a workgroup barrier between two levels.  All
//      threads stride over the level's (id, val of the child) pairs — one 8-byte load each, the root's tens of thousands
//      as any other's —; the thread that wins the LDS atomicOr test-and-set of the id's bit does the id's ONE
//      read-add-write with val - G(s).  Ids are unique within a node and the levels are barrier-separated: who writes an
//      id, and what, does not depend on timing, and the deepest node that has an out-edge with the id is the one that counts.
//   4. THE DENSE PASS, only on a row whose state holds something (G(s) != 0, uniform): every id up to <eot> whose bit is
//      clear breaks the match and gets 0 - G(s).  16-byte loads and stores, up to three ids in front of the first 16-byte
//      boundary of the row and up to three behind the last peeled off; a group of four with no bit set takes one 16-byte
//      store, a mixed group one 4-byte store per clear bit, a group the sparse pass served whole is not even loaded.
// Every id <= <eot> is written at most once, the ids above it never; a -inf logit stays -inf (-inf + finite).
// LDS: 7 312 bytes, the mask 7 172 of them; 15 VGPRs, no scratch.  SCORE = false / true: the two row forms of fwd::row_history.
// ------------------------------------------------------------------------------------
#define BGRAPH_THREADS 256
// (one word more than the ids need: the 64-bit window of the dense pass's last group reads it)
#define BGRAPH_MASK_WORDS (LP_SUP_WORDS * 2 + 1)
template <bool SCORE>
__global__ __launch_bounds__(BGRAPH_THREADS) void dec_boost_graph_kernel(float* __restrict__ logits, const int* __restrict__ tab,
                                                                        int V, int K, int R, int NT, int eot, int ts_begin,
                                                                        fwd::RowSource src) {
  __shared__ unsigned claimed[BGRAPH_MASK_WORDS];
  __shared__ int s_tl[fwd::BOOST_GRAPH_MAX_DEPTH];   // the row's last text ids, the last one first
  __shared__ int s_nt, s_state;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* hist;
  int n;
  if (!fwd::row_history<SCORE>(src, r, K, R, NT, hist, n)) return;   // (uniform, in front of the first barrier)
  const int n_ids = eot + 1;
  const int root = tab[4];

  // 1. the last text ids | the mask
  if (wv == 0) {
    int cnt = 0;
    for (int i0 = 0; i0 < n && cnt < fwd::BOOST_GRAPH_MAX_DEPTH; i0 += 64) {   // (uniform)
      const int i = n - 1 - i0 - lane;
      const int id = i >= 0 ? hist[i] : ts_begin;
      const bool text = id < ts_begin;
      const unsigned long long b = __ballot(text);
      const int at = cnt + __popcll(b & ((1ull << lane) - 1ull));
      if (text && at < fwd::BOOST_GRAPH_MAX_DEPTH) s_tl[at] = id;
      cnt += __popcll(b);
    }
    if (lane == 0) s_nt = min(cnt, fwd::BOOST_GRAPH_MAX_DEPTH);
  } else {
    const int n_words = (n_ids + 31) / 32 + 1;
    for (int w = tid - 64; w < n_words; w += BGRAPH_THREADS - 64) claimed[w] = 0u;
  }
  __syncthreads();

  // 2. the state: the deepest suffix that is a node
  if (wv == 0) {
    const int node = lane < s_nt ? fwd::boost_graph_suffix_node(tab, s_tl, lane + 1) : 0;
    const unsigned long long b = __ballot(node != 0);
    const int s = b ? __builtin_amdgcn_readlane(node, 63 - __clzll((long long)b)) : root;
    if (lane == 0) s_state = s;
  }
  __syncthreads();

  // 3. the sparse pass: s, fail(s), .. root
  const int s = __builtin_amdgcn_readfirstlane(s_state);
  const float G = fwd::ngram_bits_float(tab[s + 2]);
  float* lg = logits + (size_t)r * V;
  int node = s;
  for (int level = 0; level <= fwd::BOOST_GRAPH_MAX_DEPTH; ++level) {   // (uniform; a chain is at most 32 links)
    const int cnt = tab[node];
    const int* vals = tab + node + fwd::BOOST_GRAPH_REC_WORDS + 2 * cnt;
    for (int e = tid; e < cnt; e += BGRAPH_THREADS) {
      const int2 p = *reinterpret_cast<const int2*>(vals + 2 * e);
      if ((unsigned)p.x >= (unsigned)n_ids) continue;   // (the callers refuse such a list: never outside the row anyway)
      const unsigned bit = 1u << (p.x & 31);
      // (a row in the root state has one level and no dense pass: nobody asks who claimed what)
      if (s == root || !(atomicOr(&claimed[p.x >> 5], bit) & bit)) lg[p.x] += fwd::boost_graph_delta(p.y, G);
    }
    if (node == root) break;
    node = __builtin_amdgcn_readfirstlane(tab[node + 1]);
    __syncthreads();
  }
  if (G == 0.0f) return;   // (uniform) nothing to take back: the ids that continue no phrase keep their bits
  __syncthreads();

  // 4. the dense pass: every unclaimed id breaks the match
  const float back = fwd::boost_graph_delta(0, G);
  const auto is_claimed = [&](int v) { return (claimed[v >> 5] >> (v & 31)) & 1u; };
  int head = (int)(((16u - (unsigned)((uintptr_t)lg & 15u)) & 15u) >> 2);   // ids in front of the first 16-byte boundary
  head = head < n_ids ? head : n_ids;
  const int n_vec = (n_ids - head) >> 2, tail0 = head + 4 * n_vec;
  if (tid < head && !is_claimed(tid)) lg[tid] += back;
  {
    const int v = tail0 + tid;   // tid < 3 at most
    if (v < n_ids && !is_claimed(v)) lg[v] += back;
  }
  for (int i = tid; i < n_vec; i += BGRAPH_THREADS) {
    const int v0 = head + 4 * i;   // v0 + 3 < tail0 <= n_ids
    const int w = v0 >> 5;
    const unsigned long long win = ((unsigned long long)claimed[w + 1] << 32) | claimed[w];
    const unsigned c4 = (unsigned)(win >> (v0 & 31)) & 15u;
    if (c4 == 15u) continue;
    float4 x = *reinterpret_cast<const float4*>(lg + v0);
    x.x += back; x.y += back; x.z += back; x.w += back;
    if (c4 == 0u) {
      *reinterpret_cast<float4*>(lg + v0) = x;
    } else {
      if (!(c4 & 1u)) lg[v0] = x.x;
      if (!(c4 & 2u)) lg[v0 + 1] = x.y;
      if (!(c4 & 4u)) lg[v0 + 2] = x.z;
      if (!(c4 & 8u)) lg[v0 + 3] = x.w;
    }
  }
}

namespace fwd {

bool boost_graph_geometry_ok(int V, int eot, int ts_begin) {
  return V >= 1 && V <= LP_SUP_WORDS * 64 && eot >= 0 && eot < ts_begin && ts_begin <= V;
}

void launch_boost_graph(hipStream_t st, const GenDev& gp, float* logits, const int* tab, const RowSource& src, int rows) {
  const bool step = src.tab == nullptr;
  if (!tab || (step ? gp.R : rows) <= 0 || !boost_graph_geometry_ok(gp.V, gp.eot, gp.ts_begin)) return;
  if (step)
    dec_boost_graph_kernel<false><<<gp.R, BGRAPH_THREADS, 0, st>>>(logits, tab, gp.V, gp.K, gp.R, gp.n_text_ctx, gp.eot,
                                                                   gp.ts_begin, src);
  else
    dec_boost_graph_kernel<true><<<rows, BGRAPH_THREADS, 0, st>>>(logits, tab, gp.V, 1, rows, gp.n_text_ctx, gp.eot,
                                                                  gp.ts_begin, src);
}

void boost_graph_rows_host(const int* tab, float* logits, int rows, int V, int eot, int ts_begin, const int* hist,
                           const int* hist_offsets) {
  if (!boost_graph_geometry_ok(V, eot, ts_begin)) return;
  const int root = tab[4];
  std::vector<char> claimed((size_t)eot + 1);
  for (int r = 0; r < rows; ++r) {
    int tl[BOOST_GRAPH_MAX_DEPTH], nt = 0;
    for (int i = hist_offsets[r + 1] - 1; i >= hist_offsets[r] && nt < BOOST_GRAPH_MAX_DEPTH; --i)
      if (hist[i] < ts_begin) tl[nt++] = hist[i];
    int s = root;
    for (int k = 1; k <= nt; ++k)
      if (const int node = boost_graph_suffix_node(tab, tl, k)) s = node;
    const float G = ngram_bits_float(tab[s + 2]);
    std::fill(claimed.begin(), claimed.end(), 0);
    float* lg = logits + (size_t)r * V;
    for (int node = s;; node = tab[node + 1]) {
      const int cnt = tab[node];
      const int* vals = tab + node + BOOST_GRAPH_REC_WORDS + 2 * cnt;
      for (int e = 0; e < cnt; ++e) {
        const int v = vals[2 * e];
        if (v < 0 || v > eot || claimed[v]) continue;
        claimed[v] = 1;
        lg[v] += boost_graph_delta(vals[2 * e + 1], G);
      }
      if (node == root) break;
    }
    if (G == 0.0f) continue;
    for (int v = 0; v <= eot; ++v)
      if (!claimed[v]) lg[v] += boost_graph_delta(0, G);
  }
}

}  // namespace fwd

extern "C" int32_t fw_boost_create_revocable(int32_t n_vocab, const int32_t* tokens, const int32_t* offsets, int32_t n_phrases,
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
    // the prefix trie, as fw_boost_create_large builds it: the phrases by their ids, lexicographically, so that the nodes
    // are numbered in pre-order (a parent in front of its children) and a node's children appear by ascending id —
    // whatever order and however often the caller named the phrases
    std::vector<int> order((size_t)n_phrases);
    for (int j = 0; j < n_phrases; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      return std::lexicographical_compare(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b], tokens + offsets[b + 1]);
    });
    std::vector<int32_t> parent(1, -1), id(1, -1), n_child(1, 0), depth(1, 0);
    std::vector<float> w(1, 0.0f);     // of node v: the largest boost through the edge that enters v
    std::vector<char> term(1, 0);      // some phrase ends at v
    int path[FW_BOOST_MAX_LEN + 1] = {0}, prev = -1;
    int top_id = -1, top_phrase = -1;  // the largest id of the list and the first phrase that holds it (for messages)
    for (int j = 0; j < n_phrases; ++j)
      for (int i = offsets[j]; i < offsets[j + 1]; ++i)
        if (tokens[i] > top_id) { top_id = tokens[i]; top_phrase = j; }
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
        float& m = w[path[d + 1]];
        if (boosts[j] > m || (boosts[j] == m && !std::signbit(boosts[j]))) m = boosts[j];
      }
      for (int d = lcp; d < L; ++d) {
        const int nn = (int)parent.size();
        parent.push_back(path[d]); id.push_back(p[d]); n_child.push_back(0); depth.push_back(d + 1);
        w.push_back(boosts[j]); term.push_back(0);
        ++n_child[path[d]];
        path[d + 1] = nn;
      }
      term[path[L]] = 1;
      prev = j;
    }
    const int n_nodes = (int)parent.size();
    std::vector<int32_t> rec((size_t)n_nodes);
    int64_t words = BOOST_GRAPH_HDR_WORDS;
    for (int i = 0; i < n_nodes; ++i) {
      rec[i] = (int32_t)words;
      words += BOOST_GRAPH_REC_WORDS + 4 * (int64_t)n_child[i];
    }
    fw_boost* b = new (std::nothrow) fw_boost();
    if (!b) { fw::set_error("out of host memory"); return FW_ENOMEM; }
    std::unique_ptr<fw_boost> hold(b);
    b->n_vocab = n_vocab;
    b->revocable = true;
    b->top_phrase = top_phrase;
    std::vector<int32_t>& tab = b->table;
    tab.assign((size_t)words, 0);
    const auto bits = [](float f) { int32_t i; memcpy(&i, &f, 4); return i; };
    const int32_t hdr[BOOST_GRAPH_HDR_WORDS] = {n_nodes - 1, n_nodes, n_vocab, BOOST_GRAPH_FORM_MARK, rec[0], top_id, 0, 0};
    std::copy(hdr, hdr + BOOST_GRAPH_HDR_WORDS, tab.begin());
    // the child pairs, for now with the child's NODE NUMBER in the record offset's place: the failure links below are
    // found by transitions over this very table.  slot[v]: where the pair that enters v sits.
    std::vector<int32_t> fill((size_t)n_nodes), slot((size_t)n_nodes, 0);
    for (int i = 0; i < n_nodes; ++i) {
      tab[rec[i]] = n_child[i];
      fill[i] = rec[i] + BOOST_GRAPH_REC_WORDS;
    }
    for (int v = 1; v < n_nodes; ++v) {   // (a node's children are created by ascending id)
      const int u = parent[v];
      slot[v] = fill[u];
      tab[slot[v]] = id[v]; tab[slot[v] + 1] = v;
      tab[slot[v] + 2 * n_child[u]] = id[v];
      fill[u] += 2;
    }
    // breadth first: a failure link points to a shallower node, so a level needs the levels above it only
    std::vector<int32_t> by_depth((size_t)n_nodes), at_depth(FW_BOOST_MAX_LEN + 2, 0);
    for (int v = 0; v < n_nodes; ++v) ++at_depth[depth[v] + 1];
    for (int d = 1; d < FW_BOOST_MAX_LEN + 2; ++d) at_depth[d] += at_depth[d - 1];
    for (int v = 0; v < n_nodes; ++v) by_depth[at_depth[depth[v]]++] = v;
    std::vector<int32_t> fail((size_t)n_nodes, 0);
    for (int v : by_depth) {
      if (depth[v] < 2) continue;   // (the root, and the nodes of one id: the only proper suffix is the empty one)
      for (int f = fail[parent[v]];; f = fail[f]) {
        if (const int c = boost_graph_child(tab.data(), rec[f], id[v])) { fail[v] = c; break; }
        if (f == 0) break;
      }
    }
    // G, C by pre-order (the parent first), E and val breadth first (the failure target first); float32, in the order of
    // include/fwamd.h
    std::vector<float> G((size_t)n_nodes, 0.0f), E((size_t)n_nodes, 0.0f);
    for (int v = 1; v < n_nodes; ++v) {
      const float through = G[parent[v]] + w[v];
      if (term[v]) E[v] = through; else G[v] = through;   // (E holds C(v) until the pass below adds E(fail(v)))
    }
    for (int v : by_depth) {
      if (v == 0) continue;
      E[v] = E[v] + E[fail[v]];
      const float val = G[v] + E[v];
      tab[slot[v] + 1] = rec[v];
      tab[slot[v] + 2 * n_child[parent[v]] + 1] = bits(val);
    }
    for (int v = 0; v < n_nodes; ++v) {
      tab[rec[v] + 1] = rec[fail[v]];
      tab[rec[v] + 2] = bits(G[v]);
    }
    *out = hold.release();
  } catch (const std::bad_alloc&) {
    fw::set_error("out of host memory");
    return FW_ENOMEM;
  }
  return FW_OK;
}
