// K17/K18 (+ the row part of K19), K22 and the scoring kernel — the decoder kernels that hold or walk ONE VOCABULARY ROW
// of float32 logits per workgroup, for gfx950: the logits rules with their log-softmax and top-C (dec_logits_process_kernel),
// the score of a given token (dec_score_kernel), and the two plain softmax probabilities (dec_nospeech_kernel,
// dec_token_prob_kernel).  The rules and the score kernel promise each other's bits for the same row: everything the two
// do alike is ONE device function below, called by both.
// dec_trunc.hip includes this file with DEC_VOCAB_TRUNC_UNIT defined: it then holds the row helpers and the kernel templates
// only, and that unit instantiates the TRUNC forms of the rules kernel (this one never does: its kernels stay the twelve
// they were).
#include "common.h"
#include "dec_kernels.h"

// ------------------------------------------------------------------------------------
// softmax(lg[0 .. V))[id] by the whole workgroup (blockDim.x <= 2048): the value is returned in thread 0, 0 elsewhere;
// `id` is read by thread 0 only.  red: 32 floats of LDS.
// ------------------------------------------------------------------------------------
static __device__ __forceinline__ float row_softmax_prob(const float* __restrict__ lg, int V, int id, float* red) {
  float mx = -3.0e38f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, lg[v]);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  float m2 = -3.0e38f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) m2 = fmaxf(m2, red[i]);
  __syncthreads();
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) s += __expf(lg[v] - m2);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return 0.f;
  float tot = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += red[i];
  return __expf(lg[id] - m2) / tot;
}

#ifndef DEC_VOCAB_TRUNC_UNIT
// K22: no-speech probability = softmax(logits at the <sot> position)[no_speech]
__global__ __launch_bounds__(1024) void dec_nospeech_kernel(const float* __restrict__ logits, int V, int row_mul,
                                                            int no_speech_id, float* __restrict__ out) {
  __shared__ float red[32];
  const int b = blockIdx.x;
  const float p = row_softmax_prob(logits + (size_t)b * row_mul * V, V, no_speech_id, red);
  if (threadIdx.x == 0) out[b] = p;
}

// per-token probability for align: p[r] = softmax(logits[r])[target[r]]
__global__ __launch_bounds__(1024) void dec_token_prob_kernel(const float* __restrict__ logits, int V,
                                                              const int* __restrict__ target, float* __restrict__ out,
                                                              int out_stride, int out_off, int row_mul) {
  __shared__ float red[32];
  const int b = blockIdx.x;
  const int t = target[b];
  const bool ok = t >= 0 && t < V;
  // (position blocks: chunk b's row of this position)
  const float p = row_softmax_prob(logits + (size_t)b * row_mul * V, V, ok ? t : 0, red);
  if (threadIdx.x == 0) out[(size_t)b * out_stride + out_off] = ok ? p : 0.f;
}
#endif  // DEC_VOCAB_TRUNC_UNIT

// ------------------------------------------------------------------------------------
// K17/K18 (+ the row part of K19): logits rules, fp32 log-softmax and the row's top-C
// candidates of cum + logp, one workgroup per row.
// Rule order: repetition penalty, no-repeat-ngram, suppress-blank (first
// step), suppress list, [min_new_tokens], timestamp rules (a)-(e), log-softmax.
// ------------------------------------------------------------------------------------
#define LP_THREADS 1024
#define LP_WAVES (LP_THREADS / 64)
#define LP_NV 56 /* values per thread kept in registers: V <= 56*1024 */
#define LP_NONE 0x7fffffff /* no id */
// counter-based Gumbel noise: murmur3 finaliser of (seed, row, step, token) -> u strictly in (0,1) -> -log(-log u).
// oracle/whisper.py::_gumbel restates the same integer hash.
static __device__ __forceinline__ float gumbel_noise(unsigned seed_lo, unsigned seed_hi, unsigned row, unsigned step,
                                                     unsigned v) {
  unsigned h = seed_lo ^ (row * 0x9E3779B9u) ^ (step * 0x85EBCA6Bu) ^ (v * 0xC2B2AE35u) ^ (seed_hi * 0x27D4EB2Fu);
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  // 23 bits: (h >> 9) + 0.5 is exact in fp32 for every h, so u stays strictly inside (0, 1) (with 24 bits the
  // top value rounds to 1.0 and the noise becomes +inf: that token would win whatever its probability)
  const float u = ((float)(h >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}

// ---- one held logits row: what dec_logits_process_kernel and dec_score_kernel do alike, stated once ----
// The row lives in registers (56 values per thread): all of its loads are issued back to back before the first use,
// the suppress list is one bit per token (one scalar 8-byte load per 64 tokens of a wave), every element-wise rule
// is a range test on uniform scalars.  Thread tid holds ids tid + i * LP_THREADS in val[i]; tid, lane and wv (the wave,
// uniform) are the caller's, and so is the LDS: `float red[4][LP_WAVES]`, the wave partials of the class maxima (text,
// timestamps) and class sums (text, timestamps), and `int sh_last_ts`, the timestamp rules' arg-max.

// the row: every load in flight at once
static __device__ __forceinline__ void lp_load_row(float (&val)[LP_NV], const float* __restrict__ lg, int V, int tid) {
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    const int v = tid + i * LP_THREADS;
    // (unconditional, clamped address: a load under `if (v < V)` becomes a branch around the load and the wait-count
    //  pass then drains vmcnt(0) after every second one — 28 dependent round trips, 71 us per row, instead of one)
    const float x = lg[v < V ? v : V - 1];
    val[i] = (v < V) ? x : -INFINITY;
  }
}

// timestamp-rule scalars (uniform) of a row whose history is hist[0 .. n): the position of the last timestamp token by a
// block arg-max through sh_last_ts (two barriers, taken only with with_ts: uniform)
struct LpTsBounds {
  int a_hi;   // ids in [0, a_hi) are forbidden
  int b_hi;   // timestamps in [ts_begin, b_hi) are forbidden
  int c_lo;   // ids >= c_lo are forbidden
};
static __device__ __forceinline__ LpTsBounds lp_ts_bounds(const int* __restrict__ hist, int n, bool with_ts,
                                                          const fwd::GenDev& gp, int& sh_last_ts, int tid) {
  const int tb = gp.ts_begin;
  LpTsBounds b = {0, tb, LP_NONE};
  if (with_ts) {
    if (tid == 0) sh_last_ts = -1;
    __syncthreads();
    if (tid < n && hist[tid] >= tb) atomicMax(&sh_last_ts, tid);   // n <= n_text_ctx <= LP_THREADS
    __syncthreads();
    const int lp = sh_last_ts;
    const bool last_ts = n >= 1 && lp == n - 1;
    const bool penult_ts = n < 2 || hist[n - 2] >= tb;
    if (lp >= 0) {
      const int last_seen = hist[lp];
      b.b_hi = (last_ts && !penult_ts) ? last_seen : last_seen + 1;
    }
    if (last_ts) {
      if (penult_ts) b.b_hi = LP_NONE;   // a closed pair: no timestamp at all
      else b.a_hi = gp.eot;              // an open one: text is forbidden, the pair has to close
    }
    if (n == 0) {
      b.a_hi = tb;                       // the first token is a timestamp
      if (gp.mits >= 0) b.c_lo = tb + gp.mits + 1;
    }
  }
  return b;
}

// The 64 tokens a wave holds in val[i] are CONSECUTIVE ids (v0 = 64 * (16 i + wave) .. v0 + 63), so every rule — the
// suppress list, the id ranges of the timestamp rules, the single ids — is one 64-bit lane mask per i.  Lane l of
// the wave builds the mask of i = l (56 lanes, once: word lp_lane_word of the suppress mask); applying mask i is then
// two v_readlane + ONE v_cndmask (the mask as the select operand) per value instead of ~12 vector compares / selects
// per value.
static __device__ __forceinline__ unsigned long long lp_below(int nb) {   // lanes [0, nb) of a wave's 64 ids
  return nb <= 0 ? 0ull : (nb >= 64 ? ~0ull : ((1ull << nb) - 1ull));
}
static __device__ __forceinline__ unsigned long long lp_span(int lo, int hi, int v0) {   // ids in [lo, hi) among v0 .. v0 + 63
  return lp_below(hi - v0) & ~lp_below(lo - v0);
}
static __device__ __forceinline__ int lp_lane_word(int lane, int wv) {
  return (lane < LP_NV ? lane : LP_NV - 1) * LP_WAVES + wv;
}
// this lane's rule word w: the suppress list, the timestamp ranges, the single ids kill_a / kill_b (-1: none) and, at the
// first position, the suppress_begin ids
static __device__ __forceinline__ unsigned long long lp_rule_word(const unsigned long long* __restrict__ sup_bits, int w,
                                                                  const LpTsBounds& b, int kill_a, int kill_b, int n,
                                                                  const fwd::GenDev& gp) {
  const int v0 = w * 64;
  unsigned long long km = sup_bits[w];
  km |= lp_below(b.a_hi - v0) | lp_span(gp.ts_begin, b.b_hi, v0) | ~lp_below(b.c_lo - v0) |
        lp_span(kill_a, kill_a + 1, v0) | lp_span(kill_b, kill_b + 1, v0);
  if (n == 0 && gp.suppress_blank) {   // first step only
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < gp.n_sup_begin) km |= lp_span(gp.sup_begin[q], gp.sup_begin[q] + 1, v0);
  }
  return km;
}
// word i of a mask that lane i holds as (lo, hi): uniform
static __device__ __forceinline__ unsigned long long lp_word_of_lane(unsigned lo, unsigned hi, int i) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, i) << 32) |
         (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, i);
}

// The masks applied to val[], then the class maxima and the class sums of exp(x - class max) (text ids below ts_begin,
// timestamps from there; exp(-inf) = 0 drops the masked ids) over the workgroup: LDS partials, reduced in a fixed order
// so that every thread agrees; two barriers.  An empty class: max -inf, sum 0.
// TXI: the first TXI values of every thread are text ids whatever the thread (ts_begin >= TXI * 1024: 48 for every
// Whisper vocabulary, 0 for the synthetic test vocabularies) — a compile-time class split, no per-lane test there.
// RULES = false: nothing is masked and every id is text (the raw distribution).  pre(i, x): the caller's own step on
// value i before its mask.
struct LpClasses { float max_t, max_s, sum_t, sum_s; };
struct LpNoPre { __device__ __forceinline__ float operator()(int, float x) const { return x; } };
template <int TXI, bool RULES, class Pre>
static __device__ __forceinline__ LpClasses lp_mask_reduce(float (&val)[LP_NV], unsigned km_lo, unsigned km_hi, int tb,
                                                           float (&red)[4][LP_WAVES], int tid, int lane, int wv, Pre pre) {
  const float NEG = -INFINITY;
  float mt = NEG, ms = NEG;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    float x = val[i];
    if (RULES) {
      x = pre(i, x);
      x = __builtin_amdgcn_inverse_ballot_w64(lp_word_of_lane(km_lo, km_hi, i)) ? NEG : x;
      val[i] = x;
    }
    if (i < TXI) mt = fmaxf(mt, x);
    else {
      const bool text = !RULES || tid + i * LP_THREADS < tb;
      mt = fmaxf(mt, text ? x : NEG);
      ms = fmaxf(ms, text ? NEG : x);
    }
  }
  mt = wave_max_v(mt);
  ms = wave_max_v(ms);
  if (lane == 0) { red[0][wv] = mt; red[1][wv] = ms; }
  __syncthreads();
  LpClasses c;
  c.max_t = red[0][0]; c.max_s = red[1][0];
#pragma unroll
  for (int i = 1; i < LP_WAVES; ++i) { c.max_t = fmaxf(c.max_t, red[0][i]); c.max_s = fmaxf(c.max_s, red[1][i]); }
  const float off_t = (c.max_t == NEG) ? 0.f : c.max_t, off_s = (c.max_s == NEG) ? 0.f : c.max_s;
  float st = 0.f, ss = 0.f;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    if (i < TXI) st += __expf(val[i] - off_t);
    else {
      const bool text = !RULES || tid + i * LP_THREADS < tb;
      const float e = __expf(val[i] - (text ? off_t : off_s));
      st += text ? e : 0.f;     // (x + 0 == x: the bits of `if (text) st += e; else ss += e;`)
      ss += text ? 0.f : e;
    }
  }
  st = wave_sum_v(st);   // the butterfly of __shfl_xor 32 .. 1 on the VALU: same partners, same bits (common.h)
  ss = wave_sum_v(ss);
  if (lane == 0) { red[2][wv] = st; red[3][wv] = ss; }
  __syncthreads();
  c.sum_t = 0.f; c.sum_s = 0.f;
#pragma unroll
  for (int i = 0; i < LP_WAVES; ++i) { c.sum_t += red[2][i]; c.sum_s += red[3][i]; }   // fixed order
  return c;
}

// Rule (e) and the log-sum-exp of what is left, in two parts: logp = (x - m) - l with m the maximum and l the log of the
// sum of exp(x - m): x - m is exact or nearly so and l is small, so logp carries the round-off of ITS OWN size.
// (x - (m + l) rounds m + l at the spacing of |m| first: 8e-6 at |m| = 128, whatever the size of logp.)
// (-inf - finite = -inf: the masked ids need no test; every id masked: nothing is subtracted, m = l = 0)
struct LpLse {
  bool mask_text;   // rule (e) fired: the text ids are masked too (uniform)
  float m, l;
};
static __device__ __forceinline__ LpLse lp_lse_split(const LpClasses& c, bool with_ts) {
  const float NEG = -INFINITY;
  const float log_t = logf(c.sum_t), log_s = logf(c.sum_s);   // (an empty class: its log is never used)
  const float lse_s = (c.max_s == NEG) ? NEG : c.max_s + log_s;
  LpLse r = {false, 0.f, 0.f};
  // rule (e): if logsumexp(timestamps) > max(text) (in log-prob space the common lse cancels): text is masked
  r.mask_text = __builtin_amdgcn_readfirstlane((with_ts && lse_s > c.max_t) ? 1 : 0) != 0;
  if (r.mask_text || c.max_t == NEG) {
    if (c.max_s != NEG) { r.m = c.max_s; r.l = log_s; }
  } else if (c.max_s == NEG) {
    r.m = c.max_t; r.l = log_t;
  } else {   // both classes alive: the class sums on the larger maximum
    const bool t_hi = c.max_t >= c.max_s;
    r.m = t_hi ? c.max_t : c.max_s;
    r.l = logf((t_hi ? c.sum_t : c.sum_s) + (t_hi ? c.sum_s : c.sum_t) * expf((t_hi ? c.max_s : c.max_t) - r.m));
  }
  return r;
}
// the log-prob of id v from its masked logit x
static __device__ __forceinline__ float lp_logp(float x, int v, int tb, const LpLse& lse) {
  if (lse.mask_text) x = (v < tb) ? -INFINITY : x;
  return (x - lse.m) - lse.l;
}

// Block arg-max of (key desc, token asc): a wave arg-max (DPP / permlane exchanges; the ds_bpermute butterfly was ~1 500
// cycles per round), the 16 wave partials through bkey_s / btok_s and ONE barrier, then lane l takes partial l % 16 and
// four exchanges inside the 16-lane row leave the winner in every lane (the relation is a total order on (key, token):
// the result does not depend on the exchange pattern).  k, t: this thread's pair in, the workgroup's out.
static __device__ __forceinline__ void lp_block_argmax(float& k, int& t, float* bkey_s, int* btok_s, int lane, int wv) {
  wave_argmax_v(k, t);
  if (lane == 0) { bkey_s[wv] = k; btok_s[wv] = t; }
  __syncthreads();
  k = bkey_s[lane & (LP_WAVES - 1)];
  t = btok_s[lane & (LP_WAVES - 1)];
  argmax_pair_step(k, t, dpp_f<FW_DPP_XOR1>(k), dpp_i<FW_DPP_XOR1>(t));
  argmax_pair_step(k, t, dpp_f<FW_DPP_XOR2>(k), dpp_i<FW_DPP_XOR2>(t));
  argmax_pair_step(k, t, dpp_f<FW_DPP_ROR4>(k), dpp_i<FW_DPP_ROR4>(t));
  argmax_pair_step(k, t, dpp_f<FW_DPP_ROR8>(k), dpp_i<FW_DPP_ROR8>(t));
}

// ---- TRUNC: the cut of a truncated draw (fw_generate_trunc; include/fwamd.h states the contract) ----
// The ids a row may draw are a PREFIX of the order (log-prob descending, id ascending), so the whole set is one pair:
// S = {v : logp[v] > cut.lp, or logp[v] == cut.lp and v <= cut.id}.  Both limits are monotone measures of a threshold t on
// the log-prob — the COUNT of ids at or above t for top-k, their tempered MASS for the nucleus — so one bisection serves
// both: over the order-preserving integer image of the fp32 value (31 rounds whatever k), which ends on the boundary
// VALUE exactly; the ids that share that value are then told apart by a second bisection over the id (16 rounds, taken
// only when the cut falls inside a tie group).  A round is one pass over the 56 registers, the 16 wave partials through
// LDS and ONE barrier (partials double-buffered).  Counts never leave the scalar unit (popcount of the compare mask);
// masses are summed per thread in ascending i, over the wave by wave_sum_v, over the waves in ascending order: a fixed
// order, no atomics, so a row gets the same cut wherever and however often it runs.  val[] is only read.
struct LpCut { float lp; int id; };
// the image: u(x) < u(y) <=> x < y over the floats without NaN; x is a log-prob here (<= 0, -inf for a masked id)
static __device__ __forceinline__ unsigned lp_img(float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x + 0.0f);   // (-0 -> +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static __device__ __forceinline__ float lp_img_inv(unsigned u) {
  return __builtin_bit_cast(float, (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
#define LP_IMG_NEG_INF 0x007FFFFFu   /* lp_img(-inf): every live value lies above */
// a float every lane agrees on, held in a scalar register (a uniform float computed on the vector unit keeps a vector
// register across the rounds)
static __device__ __forceinline__ float lp_uniform(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// workgroup totals of a per-wave scalar count / of per-thread masses; `rd` counts the rounds (their parity picks the buffer)
static __device__ __forceinline__ int lp_block_sum_i(int c, int (&part)[2][LP_WAVES], int& rd, int lane, int wv) {
  const int par = rd & 1;
  ++rd;
  if (lane == 0) part[par][wv] = c;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < LP_WAVES; ++i) t += part[par][i];
  return __builtin_amdgcn_readfirstlane(t);
}
static __device__ __forceinline__ float lp_block_sum_f(float s, int (&part)[2][LP_WAVES], int& rd, int lane, int wv) {
  const int par = rd & 1;
  ++rd;
  s = wave_sum_v(s);
  if (lane == 0) part[par][wv] = __builtin_bit_cast(int, s);
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < LP_WAVES; ++i) t += __builtin_bit_cast(float, part[par][i]);   // fixed order
  return lp_uniform(t);
}
// this wave's ids with val >= t
static __device__ __forceinline__ int lp_count_ge(const float (&val)[LP_NV], float t) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(val[i] >= t));
  return c;
}
// this thread's tempered mass exp((logp - max logp) / T) of its ids with t_lo <= val < t_hi (lmax = -max logp); a group of
// 64 ids with nothing in the window costs two compares (the window shrinks by half per round)
static __device__ __forceinline__ float lp_mass_window(const float (&val)[LP_NV], float t_lo, float t_hi, float lmax,
                                                       float inv_temp) {
  // (lmax behind an empty asm: the 56 exponents (val[i] + lmax) * inv_temp do not depend on the round, and hoisted out of
  //  the bisection they are 56 more live registers beside the row)
  asm volatile("" : "+s"(lmax));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    const bool in = val[i] >= t_lo && val[i] < t_hi;
    if (__builtin_amdgcn_ballot_w64(in) != 0ull) s += in ? __expf((val[i] + lmax) * inv_temp) : 0.f;
  }
  return s;
}
// the n-th lowest id (n >= 1, at most the group's size) among the ids with val == t
static __device__ __forceinline__ int lp_nth_id(const float (&val)[LP_NV], float t, int n, int V, int (&part)[2][LP_WAVES],
                                                int& rd, int tid, int lane, int wv) {
  int lo = -1, hi = V - 1;   // ids <= lo hold fewer than n of the group, ids <= hi at least n
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    // (t behind an empty asm: 56 compare masks `val[i] == t` hoisted out of the rounds are 112 scalar registers, which
    //  spill into vector registers and push eight values of the row into scratch)
    asm volatile("" : "+s"(t), "+v"(tid));   // (tid: likewise, the ids of these rounds are their own)
    int c = 0;
#pragma unroll
    for (int i = 0; i < LP_NV; ++i)
      // (the id test against a scalar: `tid + i * LP_THREADS <= mid` would keep 56 hoisted ids alive across the rounds)
      c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(val[i] == t && tid <= mid - i * LP_THREADS));
    if (lp_block_sum_i(c, part, rd, lane, wv) >= n) hi = mid; else lo = mid;
  }
  return hi;
}
// val[]: the row's plain log-probs; lmax: lse.l (the row's best log-prob is (m - m) - l = -l exactly); every argument but
// val and the thread's own indices is uniform, and so is every branch and trip count below.
static __device__ __forceinline__ LpCut lp_trunc_cut(const float (&val)[LP_NV], int V, float lmax_v, float inv_temp, int top_k,
                                                     float top_p, int tid, int lane, int wv) {
  __shared__ int part[2][LP_WAVES];
  const float lmax = lp_uniform(lmax_v);
  int rd = 0;
  LpCut cut = {-INFINITY, LP_NONE};   // everything that is live
  const int n_live = lp_block_sum_i(lp_count_ge(val, lp_img_inv(LP_IMG_NEG_INF + 1u)), part, rd, lane, wv);
  if (n_live == 0) return cut;
  const unsigned img_top = lp_img(-lmax) + 1u;   // above every value of the row
  // ---- top-k: the largest t with count(t) >= k, then the lowest ids of its tie group ----
  int k_need = 0;   // ids S_k takes from the tie group at cut.lp (0: no top-k cut, cut.lp = -inf)
  if (top_k >= 1 && top_k < n_live) {
    unsigned lo = LP_IMG_NEG_INF, hi = img_top;   // count(lo) >= k > count(hi)
    int c_lo = n_live, c_hi = 0;
    while (hi - lo > 1u) {
      const unsigned mid = lo + (hi - lo) / 2u;
      const int c = lp_block_sum_i(lp_count_ge(val, lp_img_inv(mid)), part, rd, lane, wv);
      if (c >= top_k) { lo = mid; c_lo = c; } else { hi = mid; c_hi = c; }
    }
    cut.lp = lp_img_inv(lo);
    k_need = top_k - c_hi;
    if (k_need < c_lo - c_hi) cut.id = lp_nth_id(val, cut.lp, k_need, V, part, rd, tid, lane, wv);
  }
  // ---- nucleus over S_k: the largest t with mass(t) >= p * Z, then as many ids of its tie group as stay below p * Z ----
  if (top_p < 1.0f) {
    const unsigned img_k = lp_img(cut.lp);
    // Z: what lies above the top-k boundary value, plus the ids S_k takes at it (equal log-probs: equal weights)
    const float w_k = k_need > 0 ? __expf((cut.lp + lmax) * inv_temp) : 0.f;
    const float Z = lp_block_sum_f(lp_mass_window(val, lp_img_inv(img_k + 1u), INFINITY, lmax, inv_temp), part, rd, lane, wv) +
                    (float)k_need * w_k;
    const float target = lp_uniform(top_p * Z);
    unsigned lo = img_k, hi = img_top;   // mass(lo) = Z >= target > mass(hi): lo itself is never evaluated
    float m_hi = 0.f, t_hi = INFINITY;   // mass(hi), and hi as a value
    while (hi - lo > 1u) {
      const unsigned mid = lo + (hi - lo) / 2u;
      const float t = lp_img_inv(mid);
      const float m = lp_uniform(m_hi + lp_block_sum_f(lp_mass_window(val, t, t_hi, lmax, inv_temp), part, rd, lane, wv));
      if (m >= target) lo = mid; else { hi = mid; m_hi = m; t_hi = t; }
    }
    // the boundary value's tie group inside S_k: g ids of weight w each, m_hi ahead of the first of them
    const float t = lp_img_inv(lo);
    int g = k_need;
    if (lo != img_k) {
      int c = 0;
#pragma unroll
      for (int i = 0; i < LP_NV; ++i) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(val[i] == t));
      g = lp_block_sum_i(c, part, rd, lane, wv);
    }
    if (lo != img_k) { cut.lp = t; cut.id = LP_NONE; }
    if (g > 0) {
      const float w = __expf((t + lmax) * inv_temp);
      const float need = ceilf((target - m_hi) / w);   // ids j = 0 .. with m_hi + j * w < target; the first is always in
      const int n_in = !(need < (float)g) ? g : (need < 1.f ? 1 : (int)need);
      if (n_in < g) cut.id = lp_nth_id(val, t, n_in, V, part, rd, tid, lane, wv);
    }
  }
  return cut;
}

// Top-C: each thread keeps its own best (key, slot); a round is one block arg-max, and only the winning thread rescans
// its 56 values.
// TXI: the compile-time class split of lp_mask_reduce.
// ALT (fw_generate_alt; instantiations of their own, the others are the code they always were): the row also writes the
// first gp.n_alt rounds of its extraction to alt_tok / alt_lp [steps][R][n_alt] at [step][r][.], from the registers
// cand_lp is written from.  Beam / greedy: max(2K, n_alt) rounds, rounds < 2K fill cand_*, rounds < n_alt fill alt_*.
// Sampling: the draw is round 0 and does NOT retire its value (nothing after it read the retired value; the token, its
// cand_val and cand_lp keep their bits), then every thread finds its best plain log-prob and n_alt plain rounds follow.
// TRUNC (fw_generate_trunc; sampling only, instantiations of their own again): the row's (top_k, top_p) come from
// trunc_tab[r]; the log-prob loop leaves the keys to a second loop, lp_trunc_cut runs between the two, and the key loop
// gives an id outside the cut no key.  The noise of an id does not depend on the cut, val[] keeps the plain log-probs, and
// what is recorded (cand_val, cand_lp, the alternatives) is read from val[] as always.  A row with (0, 1.0) skips the stage
// (uniform) and every live id gets the key the plain sampling kernel gives it: the same draw, the same bits.
template <bool SMP, int TXI, bool ALT = false, bool TRUNC = false>
__global__ __launch_bounds__(LP_THREADS) void dec_logits_process_kernel(fwd::GenDev gp, float* __restrict__ logits,
                                                                        const unsigned long long* __restrict__ sup_bits,
                                                                        const int* __restrict__ hist2,
                                                                        const float* __restrict__ cum2,
                                                                        const int* __restrict__ d_step,
                                                                        const int* __restrict__ done,
                                                                        float* __restrict__ cand_val,
                                                                        int* __restrict__ cand_tok,
                                                                        float* __restrict__ cand_lp,
                                                                        const fwd::SmpRow* __restrict__ smp_tab,
                                                                        int* __restrict__ alt_tok,
                                                                        float* __restrict__ alt_lp,
                                                                        const fwd::TruncRow* __restrict__ trunc_tab) {
  static_assert(SMP || !TRUNC, "only a sampled draw is truncated");
  __shared__ float red[4][LP_WAVES];
  __shared__ int sh_last_ts;
  __shared__ float bkey_s[2][LP_WAVES];
  __shared__ int btok_s[2][LP_WAVES];
  const int r = blockIdx.x;
  const int c = r / gp.K;
  if (done[c]) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int step = *d_step;
  const int cur = step & 1;
  const int n = step;  // tokens generated so far on this row
  const int* hist = hist2 + ((size_t)cur * gp.R + r) * gp.n_text_ctx;
  float* lg = logits + (size_t)r * gp.V;
  const int tb = gp.ts_begin;
  const float NEG = -INFINITY;

  // ---- sparse rules that touch a few ids (in HBM, before the row is pulled into registers) ----
  if (gp.rep_pen != 1.0f && n > 0) {
    for (int i = tid; i < n; i += LP_THREADS) {
      const int t = hist[i];
      bool first = true;
      for (int q = 0; q < i; ++q)
        if (hist[q] == t) { first = false; break; }
      if (first) {
        const float v = lg[t];
        lg[t] = v < 0.f ? v * gp.rep_pen : v / gp.rep_pen;
      }
    }
    __syncthreads();
  }
  if (gp.ngram > 0 && n + 1 >= gp.ngram) {
    const int k = gp.ngram;
    for (int s = tid; s + k <= n; s += LP_THREADS) {
      bool match = true;
      for (int q = 0; q < k - 1; ++q)
        if (hist[s + q] != hist[n - (k - 1) + q]) { match = false; break; }
      if (match) lg[hist[s + k - 1]] = NEG;
    }
    __syncthreads();
  }
  // ---- the row, its masks, class maxima and sums, rule (e), the log-sum-exp ----
  float val[LP_NV];
  lp_load_row(val, lg, gp.V, tid);
  const LpTsBounds tsb = lp_ts_bounds(hist, n, gp.with_ts != 0, gp, sh_last_ts, tid);
  const unsigned long long kml = lp_rule_word(sup_bits, lp_lane_word(lane, wv), tsb, (n < gp.min_new) ? gp.eot : -1,
                                              gp.with_ts ? gp.no_ts : -1, n, gp);
  const LpClasses cls = lp_mask_reduce<TXI, true>(val, (unsigned)kml, (unsigned)(kml >> 32), tb, red, tid, lane, wv, LpNoPre());
  LpLse lse = lp_lse_split(cls, gp.with_ts != 0);
  // ---- log-probs; this thread's best key ----
  float cum = cum2[(size_t)cur * gp.R + r];
  if (TRUNC) {   // (uniform values into scalar registers: the stage below needs the vector registers they would hold)
    lse.m = lp_uniform(lse.m); lse.l = lp_uniform(lse.l); cum = lp_uniform(cum);
  }
  constexpr bool smp = SMP;   // a separate instantiation: 2 x 56 inlined logf stay out of the beam / greedy kernel
  // sampling: temperature, seed and first row of this row's CALL (one uniform 16-byte load; the other instantiations
  // never touch the table).  The noise of a row depends on (seed of its call, row inside its call, step, token) only.
  fwd::SmpRow sr = {1.0f, 0u, 0u, 0};
  if (smp) sr = smp_tab[r];
  const int C = smp ? 1 : 2 * gp.K;
  float bkey = NEG;
  int bq = -1;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    const int v = tid + i * LP_THREADS;
    const float x = lp_logp(val[i], v, tb, lse);
    val[i] = x;
    if (TRUNC) continue;   // (the keys follow the cut, below)
    float key = x;
    if (smp && x != NEG) key = x * sr.inv_temp + gumbel_noise(sr.seed_lo, sr.seed_hi, (unsigned)(r - sr.row0), (unsigned)step, (unsigned)v);
    if (key > bkey) { bkey = key; bq = i; }   // ascending index: ties keep the lowest
  }
  if (TRUNC) {
    const fwd::TruncRow tr = trunc_tab[r];   // (uniform)
    LpCut cut = {NEG, LP_NONE};
    if (tr.top_k > 0 || tr.top_p < 1.0f) cut = lp_trunc_cut(val, gp.V, lse.l, sr.inv_temp, tr.top_k, tr.top_p, tid, lane, wv);
    int tid_k = tid;
    asm volatile("" : "+v"(tid_k));   // (the ids of this loop are its own: none is kept alive from the loops above)
#pragma unroll
    for (int i = 0; i < LP_NV; ++i) {
      const int v = tid_k + i * LP_THREADS;
      const float x = val[i];
      const bool in = x != NEG && (x > cut.lp || (x == cut.lp && tid_k <= cut.id - i * LP_THREADS));
      if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;   // (64 consecutive ids outside the cut: no noise is drawn for them)
      float key = NEG;
      if (in) key = x * sr.inv_temp + gumbel_noise(sr.seed_lo, sr.seed_hi, (unsigned)(r - sr.row0), (unsigned)step, (unsigned)v);
      if (key > bkey) { bkey = key; bq = i; }
    }
  }
  // ---- top-C of cum + logp: C rounds (value desc, index asc).  Sampling mode (Gumbel-max): one round on
  //      logp/T + Gumbel noise; the recorded score stays cum + logp. ----
  // ALT: round `rd` fills candidate slot rd (while rd < C) and alternative slot `ai` (while 0 <= ai < n_alt): ai = rd,
  // but rd - 1 when sampling, whose round 0 is the draw.
  const int n_alt = ALT ? gp.n_alt : 0;
  const int NR = !ALT ? C : (smp ? 1 + n_alt : (C > n_alt ? C : n_alt));
  const size_t alt0 = ALT ? ((size_t)step * gp.R + r) * n_alt : 0;
  for (int cidx = 0; cidx < NR; ++cidx) {
    const bool plain = !smp || (ALT && cidx > 0);   // a round on the log-probs themselves: the winner finds its next best
    const bool w_cand = !ALT || cidx < C;           // (uniform)
    const int ai = smp ? cidx - 1 : cidx;
    const bool w_alt = ALT && ai >= 0 && ai < n_alt;
    if (ALT && smp && cidx == 1) {   // after the draw: this thread's best plain log-prob (the draw retired nothing)
      bkey = NEG; bq = -1;
#pragma unroll
      for (int i = 0; i < LP_NV; ++i)
        if (val[i] > bkey) { bkey = val[i]; bq = i; }
    }
    float wk = bkey;
    int wt = (bq < 0) ? LP_NONE : tid + bq * LP_THREADS;
    const int par = cidx & 1;   // partials double-buffered: one barrier per round
    lp_block_argmax(wk, wt, bkey_s[par], btok_s[par], lane, wv);
    if (wt == LP_NONE) {   // nothing left on this row
      if (tid == 0) {
        if (w_cand) {
          cand_val[(size_t)r * 32 + cidx] = NEG;
          cand_tok[(size_t)r * 32 + cidx] = 0;
          if (smp) { cand_val[(size_t)r * 32 + 1] = NEG; cand_tok[(size_t)r * 32 + 1] = 0; }
          if (cand_lp) {   // (a kernel argument: uniform)
            cand_lp[(size_t)r * 32 + cidx] = NEG;
            if (smp) cand_lp[(size_t)r * 32 + 1] = NEG;
          }
        }
        if (w_alt) { alt_tok[alt0 + ai] = 0; alt_lp[alt0 + ai] = NEG; }
      }
      continue;
    }
    if ((wt & (LP_THREADS - 1)) == tid) {   // the winning thread: record, retire the value, find its next best
      const int wq = wt / LP_THREADS;
      float raw = NEG;
      bkey = NEG; bq = -1;
#pragma unroll
      for (int i = 0; i < LP_NV; ++i) {
        if (i == wq) { raw = val[i]; if (!(ALT && smp) || cidx > 0) val[i] = NEG; }
        if (plain && val[i] > bkey) { bkey = val[i]; bq = i; }
      }
      if (w_cand) {
        cand_val[(size_t)r * 32 + cidx] = cum + raw;
        cand_tok[(size_t)r * 32 + cidx] = wt;
        if (smp) { cand_val[(size_t)r * 32 + 1] = NEG; cand_tok[(size_t)r * 32 + 1] = 0; }
        // the token's own log-prob, as it was added to cum: stored, not recovered later from two running sums
        // (fl(cum + raw) - cum is not raw once |raw| > |cum|)
        if (cand_lp) {
          cand_lp[(size_t)r * 32 + cidx] = raw;
          if (smp) cand_lp[(size_t)r * 32 + 1] = NEG;
        }
      }
      if (w_alt) { alt_tok[alt0 + ai] = wt; alt_lp[alt0 + ai] = raw; }
    }
  }
}

// ------------------------------------------------------------------------------------
// Scoring (fw_score): the log-prob of a GIVEN token per logits row, with the row's arg-max beside it, one workgroup per
// row, every row of a position block in one launch.  Row r of the launch is position pos0 + r % nb of sequence r / nb and
// reads its ScoreRow (target id, history, output index) from tab[(r / nb) * tab_stride + pos0 + r % nb]; a row without
// a target (target < 0) writes nothing.
// The row is held and reduced by the helpers dec_logits_process_kernel uses, so a row scored here gets the bits that
// kernel gives the same row of a greedy decode step.  Its own five steps:
//   * RULES: the decoding rules of a greedy row whose history is hist[0 .. n) (n = the row's own position among its
//     targets: no d_step, no parity half, no min_new_tokens).  !RULES: the raw distribution, every id one class.
//   * the logits are READ ONLY.  The two sparse rules (repetition penalty, no-repeat n-gram) mark their ids in two LDS
//     bit maps laid out like the suppress mask (one 64-bit word per 64 consecutive ids a wave holds in val[i]): the
//     n-gram bits join the rule word, the penalty is applied to the register copy of the words that have a bit set.
//   * the target's value picked out of its owner's registers, one arg-max round instead of top-C, the stores.
// ------------------------------------------------------------------------------------
template <bool RULES>
__global__ __launch_bounds__(LP_THREADS) void dec_score_kernel(fwd::GenDev gp, const float* __restrict__ logits,
                                                               const unsigned long long* __restrict__ sup_bits,
                                                               const fwd::ScoreRow* __restrict__ tab, int tab_stride,
                                                               int pos0, int nb, const int* __restrict__ hist_pool,
                                                               float* __restrict__ out_lp, int* __restrict__ out_best_id,
                                                               float* __restrict__ out_best_lp) {
  __shared__ float red[4][LP_WAVES];
  __shared__ int sh_last_ts;
  __shared__ float bkey_s[LP_WAVES];
  __shared__ int btok_s[LP_WAVES];
  __shared__ unsigned pen_bits[2 * LP_SUP_WORDS], ng_bits[2 * LP_SUP_WORDS];
  const int r = blockIdx.x;
  const fwd::ScoreRow row = fwd::score_row(tab, tab_stride, pos0, nb, r);
  if (row.target < 0) return;   // (uniform)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = row.n;
  const int* hist = hist_pool + row.hist_off;
  const int tb = gp.ts_begin;
  const float NEG = -INFINITY;
  // ---- sparse rules: the ids they touch, one bit each ----
  const bool pen_on = RULES && gp.rep_pen != 1.0f && n > 0;
  const bool ng_on = RULES && gp.ngram > 0 && n + 1 >= gp.ngram;
  if (pen_on || ng_on) {
    for (int i = tid; i < 2 * LP_SUP_WORDS; i += LP_THREADS) { pen_bits[i] = 0u; ng_bits[i] = 0u; }
    __syncthreads();
    if (pen_on)
      for (int i = tid; i < n; i += LP_THREADS) {
        const int t = hist[i];
        atomicOr(&pen_bits[t >> 5], 1u << (t & 31));   // (a bit: an id is penalised once however often it occurs)
      }
    if (ng_on) {
      const int k = gp.ngram;
      for (int s = tid; s + k <= n; s += LP_THREADS) {
        bool match = true;
        for (int q = 0; q < k - 1; ++q)
          if (hist[s + q] != hist[n - (k - 1) + q]) { match = false; break; }
        if (match) {
          const int t = hist[s + k - 1];
          atomicOr(&ng_bits[t >> 5], 1u << (t & 31));
        }
      }
    }
    __syncthreads();
  }
  // ---- the row; this lane's rule word (no min_new_tokens: kill_a = -1) with the n-gram bits, and its penalty word ----
  float val[LP_NV];
  lp_load_row(val, logits + (size_t)r * gp.V, gp.V, tid);
  const bool with_ts = RULES && gp.with_ts;
  const LpTsBounds tsb = lp_ts_bounds(hist, n, with_ts, gp, sh_last_ts, tid);
  unsigned km_lo = 0u, km_hi = 0u, pm_lo = 0u, pm_hi = 0u;
  if (RULES) {
    const int w = lp_lane_word(lane, wv);
    unsigned long long km = lp_rule_word(sup_bits, w, tsb, -1, with_ts ? gp.no_ts : -1, n, gp);
    if (ng_on) km |= ((unsigned long long)ng_bits[2 * w + 1] << 32) | (unsigned long long)ng_bits[2 * w];
    km_lo = (unsigned)km; km_hi = (unsigned)(km >> 32);
    if (pen_on) { pm_lo = pen_bits[2 * w]; pm_hi = pen_bits[2 * w + 1]; }
  }
  // ---- the penalty on the register copy, then the shared masks, class reduction, rule (e) and log-sum-exp ----
  const LpClasses cls = lp_mask_reduce<0, RULES>(val, km_lo, km_hi, tb, red, tid, lane, wv, [&](int i, float x) -> float {
    if (pen_on) {
      const unsigned long long pm = lp_word_of_lane(pm_lo, pm_hi, i);
      if (pm != 0ull) {   // (a scalar: nearly every word is empty)
        const float pv = x < 0.f ? x * gp.rep_pen : x / gp.rep_pen;
        x = __builtin_amdgcn_inverse_ballot_w64(pm) ? pv : x;
      }
    }
    return x;
  });
  const LpLse lse = lp_lse_split(cls, with_ts);
  // ---- log-probs; this thread's best; the target's value ----
  const int tq = ((row.target & (LP_THREADS - 1)) == tid) ? row.target / LP_THREADS : -1;
  float bkey = NEG, tval = NEG;
  int bq = -1;
#pragma unroll
  for (int i = 0; i < LP_NV; ++i) {
    const float x = lp_logp(val[i], tid + i * LP_THREADS, tb, lse);
    if (i == tq) tval = x;
    if (x > bkey) { bkey = x; bq = i; }   // ascending index: ties keep the lowest
  }
  if (tq >= 0) out_lp[row.out] = tval;
  if (!out_best_id) return;   // (kernel arguments: uniform; both or none)
  float wk = bkey;
  int wt = (bq < 0) ? LP_NONE : tid + bq * LP_THREADS;
  lp_block_argmax(wk, wt, bkey_s, btok_s, lane, wv);
  if (tid == 0) {
    out_best_id[row.out] = (wt == LP_NONE) ? 0 : wt;   // (nothing left on the row: id 0 at -inf, as the rules kernel records it)
    out_best_lp[row.out] = (wt == LP_NONE) ? NEG : wk;
  }
}

#ifndef DEC_VOCAB_TRUNC_UNIT
namespace fwd {

void launch_nospeech(hipStream_t st, const float* logits, int V, int row_mul, int no_speech_id, float* out, int B) {
  dec_nospeech_kernel<<<B, 1024, 0, st>>>(logits, V, row_mul, no_speech_id, out);
}

void launch_logits_process(hipStream_t st, const GenDev& gp, float* logits, const unsigned long long* sup_bits,
                           const int* hist2, const float* cum2, const int* d_step, const int* done, float* cand_val,
                           int* cand_tok, float* cand_lp, const SmpRow* smp_tab, int* alt_tok, float* alt_lp,
                           const TruncRow* trunc_tab) {
  if (gp.sample && !smp_tab) return;   // (a sampling launch without its table: nothing is launched, nothing is read)
  // every Whisper vocabulary keeps its timestamp ids above 48 * 1024 (ts_begin 50 363 .. 50 365); the synthetic
  // test vocabularies do not: they take the instantiation with a per-lane class test everywhere
  const bool wide = gp.ts_begin >= 48 * LP_THREADS;
  const bool alt = gp.n_alt > 0 && alt_tok && alt_lp;
  if (gp.n_alt > 0 && !alt) return;   // (a key that says alternatives without their buffers: nothing is launched)
  if (gp.trunc && (!gp.sample || !trunc_tab)) return;   // (a key that says truncation on a launch that cannot: nothing is launched)
#define LP_GO(SMP, TXI, ALT, TRUNC) \
  dec_logits_process_kernel<SMP, TXI, ALT, TRUNC><<<gp.R, LP_THREADS, 0, st>>>(gp, logits, sup_bits, hist2, cum2, d_step, done, cand_val, cand_tok, cand_lp, smp_tab, alt_tok, alt_lp, trunc_tab)
  if (gp.trunc) {   // (the TRUNC instantiations live in dec_trunc.hip)
    launch_logits_process_trunc(st, gp, logits, sup_bits, hist2, cum2, d_step, done, cand_val, cand_tok, cand_lp, smp_tab,
                                alt ? alt_tok : nullptr, alt ? alt_lp : nullptr, trunc_tab);
  } else if (alt) {
    if (gp.sample) { if (wide) LP_GO(true, 48, true, false); else LP_GO(true, 0, true, false); }
    else { if (wide) LP_GO(false, 48, true, false); else LP_GO(false, 0, true, false); }
  } else if (gp.sample) { if (wide) LP_GO(true, 48, false, false); else LP_GO(true, 0, false, false); }
  else { if (wide) LP_GO(false, 48, false, false); else LP_GO(false, 0, false, false); }
#undef LP_GO
}

void launch_token_prob(hipStream_t st, const float* logits, int V, const int* target, float* out, int out_stride,
                       int out_off, int rows, int row_mul) {
  dec_token_prob_kernel<<<rows, 1024, 0, st>>>(logits, V, target, out, out_stride, out_off, row_mul);
}

void launch_score(hipStream_t st, const GenDev& gp, bool rules, const float* logits, const unsigned long long* sup_bits,
                  const ScoreRow* tab, int tab_stride, int pos0, int nb, int rows, const int* hist_pool, float* out_lp,
                  int* out_best_id, float* out_best_lp) {
  if (!out_best_id || !out_best_lp) { out_best_id = nullptr; out_best_lp = nullptr; }   // both or none
  if (rules) dec_score_kernel<true><<<rows, LP_THREADS, 0, st>>>(gp, logits, sup_bits, tab, tab_stride, pos0, nb, hist_pool, out_lp, out_best_id, out_best_lp);
  else dec_score_kernel<false><<<rows, LP_THREADS, 0, st>>>(gp, logits, sup_bits, tab, tab_stride, pos0, nb, hist_pool, out_lp, out_best_id, out_best_lp);
}

}  // namespace fwd
#endif  // DEC_VOCAB_TRUNC_UNIT
