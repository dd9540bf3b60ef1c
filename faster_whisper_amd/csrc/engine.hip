// libfwamd.so — host side of the MI355X Whisper engine: C ABI (include/fwamd.h), weight
// packing/upload, workspaces and the log-mel + encoder pipeline.
// The decoder / generate / align side lives in decoder.hip, the kernel test and bench hooks in hooks.hip.
//
// Reference interfaces replaced here (faster_whisper/transcribe.py): the
// ctranslate2.models.Whisper constructor (:689-698), .encode (:1400), the
// numpy FeatureExtractor call on the host (:463-467) and StorageView.from_array (:1875).
#include "engine.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <optional>
#include <type_traits>

#include "dec_kernels.h"
#include "kernels.h"

namespace fw {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int dev_alloc(void** p, size_t bytes) {
  if (bytes == 0) bytes = 256;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    *p = nullptr;
    return FW_ENOMEM;
  }
  return FW_OK;
}

// ---------------------------------------------------------------- profiling
static const char* kProfNames[PF_COUNT] = {
    "logmel", "enc_gemm", "enc_attn", "enc_layernorm", "cross_kv_gemm", "dec_gemm_qkv", "dec_gemm_dxd",
    "dec_gemm_ffn1", "dec_gemm_ffn2", "dec_self_attn", "dec_cross_attn", "dec_logits", "dec_sample", "dec_misc"};

static hipEvent_t ev_get(Prof& p) {
  if (!p.ev_pool.empty()) {
    hipEvent_t e = p.ev_pool.back();
    p.ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
ProfScope::ProfScope(Prof& p_, int fam_, double flops, double bytes, hipStream_t st_) : p(&p_), fam(fam_), st(st_) {
  if (!p->on) return;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    a = ev_get(*p);
    b = ev_get(*p);
    p->acc[fam].flops += flops;
    p->acc[fam].bytes += bytes;
    p->acc[fam].launches += 1;
  }
  (void)hipEventRecord(a, st);
}
ProfScope::~ProfScope() {
  if (!a) return;
  (void)hipEventRecord(b, st);
  std::lock_guard<std::mutex> lk(p->mu);
  p->pending.push_back({a, b, fam});
}
void prof_collect(Prof& p) {
  // the events are waited for outside the lock (a reader may ask for the totals meanwhile)
  std::vector<Prof::PendingEv> todo;
  {
    std::lock_guard<std::mutex> lk(p.mu);
    todo.swap(p.pending);
  }
  std::vector<std::pair<int, float>> got;
  for (auto& e : todo) {
    (void)hipEventSynchronize(e.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e.a, e.b);
    got.push_back({e.fam, ms});
  }
  std::lock_guard<std::mutex> lk(p.mu);
  for (auto& g : got) p.acc[g.first].ms += g.second;
  for (auto& e : todo) {
    p.ev_pool.push_back(e.a);
    p.ev_pool.push_back(e.b);
  }
}
Prof::~Prof() {
  for (auto& e : pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto e : ev_pool) (void)hipEventDestroy(e);
}
template <typename F>   // f on the model's recorder and on every decode lane's
static void for_each_prof(Model* m, F&& f) {
  f(m->prof);
  for (auto& l : m->lanes) f(l->prof);
}

// ---------------------------------------------------------------- blob packing
struct PackItem {
  std::string name;
  int dtype, ndim;             // dtype as in BlobEntry
  int64_t dims[4] = {1, 1, 1, 1};
  std::vector<uint16_t> data;  // fp16 payload (dtype 1)
  std::vector<float> fdata;    // fp32 payload (dtype 0)
  std::vector<int8_t> qdata;   // int8 payload (dtype 2)
  PackItem(std::string name_, int dtype_, std::initializer_list<int64_t> dims_)   // a zero payload of dims_
      : name(std::move(name_)), dtype(dtype_), ndim((int)dims_.size()) {
    size_t n = 1;
    std::copy(dims_.begin(), dims_.end(), dims);
    for (int64_t x : dims_) n *= (size_t)x;
    if (dtype == 1) data.resize(n); else if (dtype == 2) qdata.resize(n); else fdata.resize(n);
  }
  const void* bytes() const {
    return dtype == 1 ? (const void*)data.data() : dtype == 2 ? (const void*)qdata.data() : (const void*)fdata.data();
  }
  int64_t nbytes() const {
    return dtype == 1 ? (int64_t)data.size() * 2 : dtype == 2 ? (int64_t)qdata.size() : (int64_t)fdata.size() * 4;
  }
};

static const fw_weight* find_w(const fw_weight* w, int n, const std::string& name) {
  for (int i = 0; i < n; ++i)
    if (name == w[i].name) return &w[i];
  return nullptr;
}
static int64_t numel(const fw_weight* w) {
  int64_t n = 1;
  for (int i = 0; i < w->ndim; ++i) n *= w->dims[i];
  return n;
}
static float w_at(const fw_weight* w, int64_t i) {
  if (w->dtype == FW_DT_F32) return reinterpret_cast<const float*>(w->data)[i];
  half_t h;
  memcpy(&h, reinterpret_cast<const uint16_t*>(w->data) + i, 2);
  return (float)h;
}
static void to_f16(const fw_weight* w, std::vector<uint16_t>& out) {
  const int64_t n = numel(w);
  out.resize(n);
  if (w->dtype == FW_DT_F16) {
    memcpy(out.data(), w->data, n * 2);
  } else {
    const float* s = reinterpret_cast<const float*>(w->data);
    for (int64_t i = 0; i < n; ++i) out[i] = f32_to_f16_bits(s[i]);
  }
}

static int expect_shape(const fw_weight* w, const std::string& name, std::initializer_list<int64_t> dims) {
  if (!w) {
    set_error("missing weight '%s'", name.c_str());
    return FW_EINVAL;
  }
  if ((size_t)w->ndim != dims.size()) {
    set_error("weight '%s': expected %zu dims, got %d", name.c_str(), dims.size(), w->ndim);
    return FW_EINVAL;
  }
  int i = 0;
  for (int64_t d : dims) {
    if (w->dims[i] != d) {
      set_error("weight '%s': dim %d is %lld, expected %lld", name.c_str(), i, (long long)w->dims[i], (long long)d);
      return FW_EINVAL;
    }
    ++i;
  }
  return FW_OK;
}

static int check_config(const fw_config* c) {
  FW_CHECK_ARG(c->n_mels > 0 && c->n_mels <= 128, "n_mels must be in (0,128], got %d", c->n_mels);
  FW_CHECK_ARG(c->d_model % 128 == 0 && c->d_model >= 128 && c->d_model <= 1280,
               "d_model must be a multiple of 128 in [128,1280], got %d", c->d_model);
  FW_CHECK_ARG(c->n_heads * 64 == c->d_model, "head dim must be 64 (n_heads=%d, d_model=%d)", c->n_heads, c->d_model);
  FW_CHECK_ARG(c->n_audio_ctx == 1500, "n_audio_ctx must be 1500, got %d", c->n_audio_ctx);
  FW_CHECK_ARG(c->n_text_ctx > 0 && c->n_text_ctx <= 448, "n_text_ctx must be in (0,448]");
  FW_CHECK_ARG(c->n_enc_layers > 0 && c->n_dec_layers > 0, "layer counts must be positive");
  FW_CHECK_ARG(c->n_vocab > c->tok_timestamp_begin && c->tok_timestamp_begin > 0, "bad vocabulary layout");
  FW_CHECK_ARG(c->n_align_heads >= 0 && c->n_align_heads <= FW_MAX_ALIGN_HEADS, "too many alignment heads");
  FW_CHECK_ARG(c->n_suppress_begin >= 0 && c->n_suppress_begin <= 8, "n_suppress_begin out of range");
  // the logits-rules kernel keeps a row's logits in registers: 56 values x 1024 threads
  FW_CHECK_ARG(c->n_vocab <= 57344, "n_vocab %d exceeds the 57344 ids the logits kernel holds per row", c->n_vocab);
  const int toks[] = {c->tok_eot, c->tok_sot, c->tok_translate, c->tok_transcribe, c->tok_sot_lm, c->tok_sot_prev,
                      c->tok_no_speech, c->tok_no_timestamps, c->tok_timestamp_begin};
  for (int t : toks) FW_CHECK_ARG(t >= 0 && t < c->n_vocab, "special token id %d outside the vocabulary of %d", t, c->n_vocab);
  FW_CHECK_ARG(c->n_langs >= 0 && c->tok_lang_begin >= 0 && c->tok_lang_begin + c->n_langs <= c->n_vocab,
               "language ids [%d, %d) outside the vocabulary of %d", c->tok_lang_begin, c->tok_lang_begin + c->n_langs,
               c->n_vocab);
  for (int i = 0; i < c->n_suppress_begin; ++i)
    FW_CHECK_ARG(c->suppress_begin[i] >= 0 && c->suppress_begin[i] < c->n_vocab, "suppress_begin id out of range");
  return FW_OK;
}

// ---------------------------------------------------------------- the weight list
// FWAMD_LN_UNFOLD (a diagnostic, default off: DESIGN.md section 5; Model::ln_unfold): 0, 1 or 2.  Set at PACK time (or
// FWAMD_PACK_PLAIN=1: the probe packs once and creates models in all three orders) the fp16 blob also carries the plain
// weights + LayerNorms of qkv / cross.q / ffn1 / the vocabulary projection (+1 GB at large-v3) for the explicit-LayerNorm
// evaluation order; without it only the folded forms travel.
static int env_ln_unfold() {
  const char* e = getenv("FWAMD_LN_UNFOLD");
  return e && e[0] >= '0' && e[0] <= '2' && !e[1] ? e[0] - '0' : 0;
}
static bool env_pack_plain() {
  const char* e = getenv("FWAMD_PACK_PLAIN");
  return env_ln_unfold() > 0 || (e && e[0] == '1');
}

// How a 2-D weight is stored: row-major [N][K]; fragment-major (engine.h: frag_pos) like the six per-layer decoder
// linears, N % 32 == 0; fragment-major with N padded to a whole 16-row tile by zero rows (the vocabulary projection); or,
// for the token embedding of an int8 model, row-major fp16 holding the de-quantised int8 rows.
enum WForm { W_ROWS, W_FRAG, W_FRAG_PAD, W_TIED_I8 };
static int64_t stored_rows(int64_t N, WForm f) { return f == W_FRAG || f == W_FRAG_PAD ? (N + 15) / 16 * 16 : N; }
// rows [r0, r0 + n) of a row-major linear, as a linear of their own
static LinearW rows_of(const LinearW& L, int r0, int n) {
  LinearW o = L;
  o.N = n;
  if (o.w) o.w += (size_t)r0 * L.K;
  if (o.wq) o.wq += (size_t)r0 * L.K;
  if (o.wscale) o.wscale += r0;
  if (o.b) o.b += r0;
  return o;
}

// THE weight list of a model: every tensor of a blob in blob order — name, shape, form for the compute type, layout, and
// the place in W that points at it.  The packer (Packer: builds the tensors from the caller's weights) and the binder
// (Binder: checks a blob's entries against the list and points W into the blob) are its two visitors:
//   v.plain(name, dims, &dst, form, src)        fp16 `name`: the caller's weight `src` (default: `name`) in `form`
//   v.conv(base, cout, cin, cin_pad, L)         <base>.wg [cout][3 * cin_pad]: the caller's <base>.w [cout][cin][3] in
//                                               GEMM form [out][tap * cin_pad + cin]; and the bias <base>.b
//   v.folded(out, wname, bname, ln, N, K, form, L)   <out>.wf / .s1 / .cf: LayerNorm `ln` folded into W (Packer::folded)
//   v.quant(out, wname, N, K, form, L)          <out>.wq / .ws: W quantised per output row (Packer::quant)
// A visitor that returns non-zero ends the walk.
template <typename V>
static int walk_weights(const fw_config& c, bool i8, bool with_plain, Weights& W, V& v) {
  const int d = c.d_model, NV = c.n_vocab;
  int rc;
#define TRY(x) do { if ((rc = (x))) return rc; } while (0)
  auto shaped = [](int N, int K) { LinearW L; L.N = N; L.K = K; return L; };
  auto conv = [&](const std::string& base, int cout, int cin, int cin_pad, LinearW& L) {
    L = shaped(cout, 3 * cin_pad);
    return v.conv(base, cout, cin, cin_pad, L);
  };
  auto ln = [&](const std::string& base, LNW& L) -> int {
    if (int r = v.plain(base + ".g", {d}, &L.g)) return r;
    return v.plain(base + ".b", {d}, &L.b);
  };
  // a linear layer: fp16 weight <base>.w, or int8 <base>.wq + scale <base>.ws in int8_float16 mode; fp16 bias <base>.b
  auto linear = [&](const std::string& base, int N, int K, WForm form, LinearW& L) -> int {
    L = shaped(N, K);
    int r = i8 ? v.quant(base, base + ".w", N, K, form, L) : v.plain(base + ".w", {N, K}, &L.w, form);
    return r ? r : v.plain(base + ".b", {N}, &L.b);
  };
  // a decoder linear fed by a LayerNorm (decoder rows are few, so the LN kernel would be pure launch overhead): fp16:
  // folded into L — and with_plain the plain linear Lp and the LayerNorm beside it; int8: the plain linear L and the
  // LayerNorm, which the row quantiser applies
  auto ln_linear = [&](const std::string& base, const std::string& lnb, int N, int K, LinearW& L, LinearW& Lp,
                       LNW& lnw) -> int {
    if (!i8) {
      L = shaped(N, K);
      int r = v.folded(base, base + ".w", base + ".b", lnb, N, K, W_FRAG, L);
      if (r || !with_plain) return r;
    }
    int r = linear(base, N, K, W_FRAG, i8 ? L : Lp);
    return r ? r : ln(lnb, lnw);
  };
  W.c_pad = ((c.n_mels + 63) / 64) * 64;
  TRY(conv("enc.conv1", d, c.n_mels, W.c_pad, W.conv1));
  TRY(conv("enc.conv2", d, d, d, W.conv2));
  TRY(v.plain("enc.pos", {c.n_audio_ctx, d}, &W.enc_pos));
  W.enc.assign(c.n_enc_layers, EncLayerW());
  W.dec.assign(c.n_dec_layers, DecLayerW());
  char nb[96];
  for (int i = 0; i < c.n_enc_layers; ++i) {
    EncLayerW& L = W.enc[i];
    auto nm = [&](const char* s) { snprintf(nb, sizeof(nb), "enc.%d.%s", i, s); return std::string(nb); };
    LinearW qkv;   // fused: Q | K rows [0, 2d) and V rows [2d, 3d) bind separately
    TRY(ln(nm("ln1"), L.ln1));
    TRY(linear(nm("attn.qkv"), 3 * d, d, W_ROWS, qkv));
    L.qk = rows_of(qkv, 0, 2 * d);
    L.v = rows_of(qkv, 2 * d, d);
    TRY(linear(nm("attn.out"), d, d, W_ROWS, L.out));
    TRY(ln(nm("ln2"), L.ln2));
    TRY(linear(nm("ffn1"), 4 * d, d, W_ROWS, L.ffn1));
    TRY(linear(nm("ffn2"), d, 4 * d, W_ROWS, L.ffn2));
  }
  TRY(ln("enc.ln_post", W.enc_ln_post));
  // [CT2-ext] int8: the token embedding shares the int8 projection weight: a lookup returns the de-quantised row
  TRY(v.plain("dec.tok_emb", {NV, d}, &W.tok_emb, i8 ? W_TIED_I8 : W_ROWS));
  TRY(v.plain("dec.pos", {c.n_text_ctx, d}, &W.dec_pos));
  for (int i = 0; i < c.n_dec_layers; ++i) {
    DecLayerW& L = W.dec[i];
    auto nm = [&](const char* s) { snprintf(nb, sizeof(nb), "dec.%d.%s", i, s); return std::string(nb); };
    LinearW ckv;   // fused, and a "many rows" GEMM operand (row-major): K rows [0, d), V rows [d, 2d)
    TRY(ln_linear(nm("self.qkv"), nm("ln1"), 3 * d, d, L.qkv, L.qkv_p, L.ln1));
    TRY(linear(nm("self.out"), d, d, W_FRAG, L.out));
    TRY(ln_linear(nm("cross.q"), nm("ln2"), d, d, L.cq, L.cq_p, L.ln2));
    TRY(linear(nm("cross.kv"), 2 * d, d, W_ROWS, ckv));
    L.ck = rows_of(ckv, 0, d);
    L.cv = rows_of(ckv, d, d);
    TRY(linear(nm("cross.out"), d, d, W_FRAG, L.cout));
    TRY(ln_linear(nm("ffn1"), nm("ln3"), 4 * d, d, L.ffn1, L.ffn1_p, L.ln3));
    TRY(linear(nm("ffn2"), d, 4 * d, W_FRAG, L.ffn2));
  }
  // the vocabulary projection: the tied embedding, quantised (int8) or with the final LayerNorm folded in (fp16)
  W.logits = shaped(NV, d);
  if (i8) {
    TRY(v.quant("dec.logits", "dec.tok_emb", NV, d, W_FRAG_PAD, W.logits));
    TRY(ln("dec.ln", W.dec_ln));
  } else {
    TRY(v.folded("dec.logits", "dec.tok_emb", "", "dec.ln", NV, d, W_FRAG_PAD, W.logits));
    if (with_plain) {
      // the explicit order: final LayerNorm as a kernel, then the tied embedding itself (fragment-major copy)
      W.logits_p = shaped(NV, d);
      TRY(v.plain("dec.logits.wp", {NV, d}, &W.logits_p.w, W_FRAG_PAD, "dec.tok_emb"));
      TRY(ln("dec.ln", W.dec_ln));
    }
  }
#undef TRY
  return FW_OK;
}

// ---------------------------------------------------------------- blob packing
// The tensor as stored fragment-major; pad_rows: N is padded to a whole tile with zero rows (dims[0] = the stored extent).
static int to_frag_major(PackItem& it, bool pad_rows) {
  const int64_t N = it.dims[0], K = it.dims[1], KE = it.dtype == 2 ? 64 : 32;
  if ((!pad_rows && N % 32) || K % KE) {
    set_error("fragment-major packing needs N %% 32 == 0 and K %% %lld == 0 (%s is %lld x %lld)", (long long)KE,
              it.name.c_str(), (long long)N, (long long)K);
    return FW_EINVAL;
  }
  const int64_t NP = stored_rows(N, W_FRAG);
  it.dims[0] = NP;
  auto permute = [&](auto& v) {
    std::remove_reference_t<decltype(v)> src;
    src.swap(v);
    v.assign((size_t)NP * K, 0);
    for (int64_t n = 0; n < N; ++n)
      for (int64_t k = 0; k < K; ++k) v[frag_pos(n, k, K, (int)KE)] = src[n * K + k];
  };
  if (it.dtype == 2) permute(it.qdata); else permute(it.data);
  return FW_OK;
}

// The packing visitor of the weight list: builds every tensor, in its final kernel layout, from the caller's weights.
struct Packer {
  const fw_weight* w;
  int nw;
  std::vector<PackItem> items;
  int source(const std::string& name, std::initializer_list<int64_t> dims, const fw_weight** t) const {
    *t = find_w(w, nw, name);
    return expect_shape(*t, name, dims);
  }
  int push(PackItem&& it, WForm form) {
    if (form == W_FRAG || form == W_FRAG_PAD)
      if (int rc = to_frag_major(it, form == W_FRAG_PAD)) return rc;
    items.push_back(std::move(it));
    return FW_OK;
  }
  int plain(const std::string& name, std::initializer_list<int64_t> dims, const half_t**, WForm form = W_ROWS,
            const char* src = nullptr) {
    const fw_weight* t;
    if (int rc = source(src ? src : name, dims, &t)) return rc;
    PackItem it(name, 1, dims);
    to_f16(t, it.data);
    if (form == W_TIED_I8) {
      const int64_t N = it.dims[0], K = it.dims[1];
      for (int64_t n = 0; n < N; ++n) {
        float amax = 0.f;
        for (int64_t k = 0; k < K; ++k) amax = std::max(amax, fabsf(f16_bits_to_f32(it.data[n * K + k])));
        const float sc = amax > 0.f ? 127.0f / amax : 0.f, ds = amax > 0.f ? amax / 127.0f : 1.0f;
        for (int64_t k = 0; k < K; ++k)
          it.data[n * K + k] = f32_to_f16_bits((float)lrintf(f16_bits_to_f32(it.data[n * K + k]) * sc) * ds);
      }
    }
    return push(std::move(it), form);
  }
  int conv(const std::string& base, int cout, int cin, int cin_pad, LinearW&) {
    const fw_weight* t;
    if (int rc = source(base + ".w", {cout, cin, 3}, &t)) return rc;
    PackItem it(base + ".wg", 1, {cout, 3 * cin_pad});
    for (int o = 0; o < cout; ++o)
      for (int c = 0; c < cin; ++c)
        for (int k = 0; k < 3; ++k)
          it.data[(size_t)o * 3 * cin_pad + (size_t)k * cin_pad + c] =
              f32_to_f16_bits(w_at(t, ((int64_t)o * cin + c) * 3 + k));
    items.push_back(std::move(it));
    return plain(base + ".b", {cout}, nullptr);
  }
  // LayerNorm folded into the consuming linear:   y = W (g*(x-mu)*rstd + b) + bias
  //                                                 = rstd * ( (W.g) x - mu * s1 ) + cf,   s1 = rowsum(W.g), cf = W b + bias
  // emits  <out>.wf [N][K] fp16 (W.g),  <out>.s1 [N] f32,  <out>.cf [N] f32
  int folded(const std::string& out, const std::string& wname, const std::string& bname, const std::string& ln, int N,
             int K, WForm form, LinearW&) {
    const fw_weight *W, *G, *LB, *Bi = nullptr;
    int rc;
    if ((rc = source(wname, {N, K}, &W)) || (rc = source(ln + ".g", {K}, &G)) || (rc = source(ln + ".b", {K}, &LB)) ||
        (!bname.empty() && (rc = source(bname, {N}, &Bi))))
      return rc;
    std::vector<float> g(K), lb(K);
    for (int k = 0; k < K; ++k) {
      g[k] = f16_bits_to_f32(f32_to_f16_bits(w_at(G, k)));
      lb[k] = f16_bits_to_f32(f32_to_f16_bits(w_at(LB, k)));
    }
    PackItem wf(out + ".wf", 1, {N, K}), s1(out + ".s1", 0, {N}), cf(out + ".cf", 0, {N});
    for (int n = 0; n < N; ++n) {
      double a1 = 0.0, ac = 0.0;
      for (int k = 0; k < K; ++k) {
        const float wv = f16_bits_to_f32(f32_to_f16_bits(w_at(W, (int64_t)n * K + k)));
        const uint16_t wg = f32_to_f16_bits(wv * g[k]);
        wf.data[(size_t)n * K + k] = wg;
        a1 += (double)f16_bits_to_f32(wg);
        ac += (double)wv * (double)lb[k];
      }
      if (Bi) ac += (double)f16_bits_to_f32(f32_to_f16_bits(w_at(Bi, n)));
      s1.fdata[n] = (float)a1;
      cf.fdata[n] = (float)ac;
    }
    if ((rc = push(std::move(wf), form))) return rc;
    items.push_back(std::move(s1));
    items.push_back(std::move(cf));
    return FW_OK;
  }
  // int8_float16 (K25, [CT2-ext] CTranslate2 convention): per output row n, scale = 127 / absmax(W[n,:]),
  // Wq = rint(W * scale) (round-half-even); the engine stores the DE-quantisation factor absmax / 127.
  // emits <out>.wq [N][K] int8 and <out>.ws [N] f32
  int quant(const std::string& out, const std::string& wname, int N, int K, WForm form, LinearW&) {
    const fw_weight* W;
    if (int rc = source(wname, {N, K}, &W)) return rc;
    PackItem wq(out + ".wq", 2, {N, K}), ws(out + ".ws", 0, {N});
    std::vector<float> row(K);
    for (int n = 0; n < N; ++n) {
      for (int k = 0; k < K; ++k) row[k] = f16_bits_to_f32(f32_to_f16_bits(w_at(W, (int64_t)n * K + k)));
      ws.fdata[n] = quant_row_i8(row.data(), K, wq.qdata.data(), [&](int k) { return (size_t)n * K + k; });
    }
    if (int rc = push(std::move(wq), form)) return rc;
    items.push_back(std::move(ws));
    return FW_OK;
  }
};

// Build the device blob image on the host: all tensors in their final kernel layouts.
static int pack_blob(const fw_config* cfg, const fw_weight* w, int nw, int compute_type,
                     std::vector<uint8_t>& blob) {
  Packer pk{w, nw, {}};
  Weights unbound;
  if (int rc = walk_weights(*cfg, compute_type == FW_COMPUTE_INT8_FLOAT16, env_pack_plain(), unbound, pk)) return rc;
  const std::vector<PackItem>& items = pk.items;
  const int64_t hdr = (int64_t)sizeof(BlobHeader) + (int64_t)items.size() * sizeof(BlobEntry);
  int64_t off = (hdr + 255) / 256 * 256;
  std::vector<BlobEntry> entries(items.size());
  for (size_t i = 0; i < items.size(); ++i) {
    BlobEntry& e = entries[i];
    memset(&e, 0, sizeof(e));
    snprintf(e.name, sizeof(e.name), "%s", items[i].name.c_str());
    e.dtype = items[i].dtype;
    e.ndim = items[i].ndim;
    for (int k = 0; k < 4; ++k) e.dims[k] = items[i].dims[k];
    e.offset = off;
    e.nbytes = items[i].nbytes();
    off = (off + e.nbytes + 255) / 256 * 256;
  }
  blob.assign((size_t)off, 0);
  BlobHeader h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, FW_BLOB_MAGIC, 8);
  h.version = 1;
  h.n_tensors = (int32_t)items.size();
  h.total_bytes = off;
  h.compute_type = compute_type;
  h.reserved = kBlobGeneration;
  h.cfg = *cfg;
  memcpy(blob.data(), &h, sizeof(h));
  memcpy(blob.data() + sizeof(h), entries.data(), entries.size() * sizeof(BlobEntry));
  for (size_t i = 0; i < items.size(); ++i)
    memcpy(blob.data() + entries[i].offset, items[i].bytes(), (size_t)entries[i].nbytes);
  return FW_OK;
}

// ---------------------------------------------------------------- blob checking and binding
// layout generation (BlobHeader::reserved): 4 = decoder linears and the vocabulary projection fragment-major; 5 = fp16
// blobs carry the plain (LayerNorm-explicit) forms of qkv / cross.q / ffn1 / logits next to the folded ones; 6 = only
// when packed with FWAMD_LN_UNFOLD set
int check_blob_header(const BlobHeader& h, int64_t blob_bytes) {
  FW_CHECK_ARG(memcmp(h.magic, FW_BLOB_MAGIC, 8) == 0 && h.version == 1, "bad weight blob magic/version");
  FW_CHECK_ARG(h.total_bytes <= blob_bytes, "weight blob truncated (%lld > %lld)", (long long)h.total_bytes,
               (long long)blob_bytes);
  FW_CHECK_ARG(h.n_tensors >= 0 && (int64_t)sizeof(h) + h.n_tensors * (int64_t)sizeof(BlobEntry) <= h.total_bytes,
               "weight blob: %d tensor entries do not fit its %lld bytes", h.n_tensors, (long long)h.total_bytes);
  if (int rc = check_config(&h.cfg)) return rc;
  FW_CHECK_ARG(h.compute_type == FW_COMPUTE_FLOAT16 || h.compute_type == FW_COMPUTE_INT8_FLOAT16,
               "unsupported compute type %d", h.compute_type);
  FW_CHECK_ARG(h.reserved == kBlobGeneration,
               "weight blob was packed by an older libfwamd (layout generation %d, expected %d): repack it", h.reserved,
               kBlobGeneration);
  return FW_OK;
}

// The binding visitor of the weight list: every tensor is looked up in the blob's entries and compared with what the
// list says of it BEFORE a pointer into the blob is formed.
struct Binder {
  const BlobHeader& h;
  char* blob;
  std::map<std::string, const BlobEntry*> by_name;
  template <typename T>
  int get(const std::string& name, int dtype, std::initializer_list<int64_t> dims, const T** out) const {
    auto it = by_name.find(name);
    FW_CHECK_ARG(it != by_name.end(), "weight blob lacks tensor '%s'", name.c_str());
    const BlobEntry& e = *it->second;
    const char* nm = name.c_str();
    FW_CHECK_ARG(e.dtype == dtype, "weight blob tensor '%s': dtype %d, expected %d", nm, e.dtype, dtype);
    FW_CHECK_ARG(e.ndim == (int)dims.size(), "weight blob tensor '%s': %d dims, expected %zu", nm, e.ndim, dims.size());
    int64_t bytes = dtype == 1 ? 2 : dtype == 2 ? 1 : 4;
    int i = 0;
    for (int64_t x : dims) {
      FW_CHECK_ARG(e.dims[i] == x, "weight blob tensor '%s': dim %d is %lld, expected %lld", nm, i, (long long)e.dims[i],
                   (long long)x);
      bytes *= x;
      ++i;
    }
    FW_CHECK_ARG(e.nbytes == bytes, "weight blob tensor '%s': %lld bytes, its shape has %lld", nm, (long long)e.nbytes,
                 (long long)bytes);
    FW_CHECK_ARG(e.offset >= 0 && e.offset % 256 == 0 && e.offset <= h.total_bytes - bytes,
                 "weight blob tensor '%s': offset %lld (%lld bytes) misaligned or outside the blob's %lld bytes", nm,
                 (long long)e.offset, (long long)bytes, (long long)h.total_bytes);
    *out = reinterpret_cast<const T*>(blob + e.offset);
    return FW_OK;
  }
  int plain(const std::string& name, std::initializer_list<int64_t> dims, const half_t** dst, WForm form = W_ROWS,
            const char* = nullptr) const {
    if (dims.size() != 2) return get(name, 1, dims, dst);
    return get(name, 1, {stored_rows(dims.begin()[0], form), dims.begin()[1]}, dst);
  }
  int conv(const std::string& base, int cout, int, int cin_pad, LinearW& L) const {
    if (int rc = get(base + ".wg", 1, {cout, 3 * cin_pad}, &L.w)) return rc;
    return get(base + ".b", 1, {cout}, &L.b);
  }
  int folded(const std::string& out, const std::string&, const std::string&, const std::string&, int N, int K,
             WForm form, LinearW& L) const {
    int rc;
    if ((rc = get(out + ".wf", 1, {stored_rows(N, form), K}, &L.w)) || (rc = get(out + ".s1", 0, {N}, &L.s1))) return rc;
    return get(out + ".cf", 0, {N}, &L.cf);
  }
  int quant(const std::string& out, const std::string&, int N, int K, WForm form, LinearW& L) const {
    if (int rc = get(out + ".wq", 2, {stored_rows(N, form), K}, &L.wq)) return rc;
    return get(out + ".ws", 0, {N}, &L.wscale);
  }
};

int bind_weights(const BlobHeader& h, const BlobEntry* entries, void* blob, Weights& W, bool* has_plain) {
  Binder b{h, reinterpret_cast<char*>(blob), {}};
  for (int i = 0; i < h.n_tensors; ++i)
    b.by_name[std::string(entries[i].name, strnlen(entries[i].name, sizeof(entries[i].name)))] = &entries[i];
  const bool i8 = h.compute_type == FW_COMPUTE_INT8_FLOAT16;
  *has_plain = !i8 && b.by_name.count("dec.logits.wp") != 0;   // packed with FWAMD_LN_UNFOLD: the explicit-LayerNorm forms travel too
  return walk_weights(h.cfg, i8, *has_plain, W, b);
}

// ---------------------------------------------------------------- mel constants
// get_mel_filters (feature_extractor.py:25-65), in double like numpy, stored float32.
static void compute_mel_filters(int n_mels, std::vector<float>& filt /* [n_mels][201] */) {
  const int n_fft = 400, nb = 201;
  const double sr = 16000.0;
  std::vector<double> fftfreqs(nb);
  const double val = 1.0 / (n_fft * (1.0 / sr));
  for (int k = 0; k < nb; ++k) fftfreqs[k] = k * val;
  const double max_mel = 45.245640471924965;
  const int n = n_mels + 2;
  std::vector<double> mels(n), freqs(n);
  const double step = (max_mel - 0.0) / (n - 1);
  for (int i = 0; i < n; ++i) mels[i] = i * step + 0.0;
  mels[n - 1] = max_mel;
  const double f_sp = 200.0 / 3;
  const double min_log_hz = 1000.0, min_log_mel = (min_log_hz - 0.0) / f_sp;
  const double logstep = log(6.4) / 27.0;
  for (int i = 0; i < n; ++i) {
    freqs[i] = 0.0 + f_sp * mels[i];
    if (mels[i] >= min_log_mel) freqs[i] = min_log_hz * exp(logstep * (mels[i] - min_log_mel));
  }
  filt.assign((size_t)n_mels * nb, 0.f);
  for (int i = 0; i < n_mels; ++i) {
    const double fd0 = freqs[i + 1] - freqs[i], fd1 = freqs[i + 2] - freqs[i + 1];
    const double enorm = 2.0 / (freqs[i + 2] - freqs[i]);
    for (int k = 0; k < nb; ++k) {
      const double lower = -(freqs[i] - fftfreqs[k]) / fd0;
      const double upper = (freqs[i + 2] - fftfreqs[k]) / fd1;
      double wv = std::max(0.0, std::min(lower, upper));
      wv *= enorm;
      filt[(size_t)i * nb + k] = (float)wv;
    }
  }
}

static int setup_logmel_consts(Model* m) {
  std::vector<float> consts(800);
  for (int j = 0; j < 400; ++j) consts[j] = (float)cos(2.0 * M_PI * (double)j / 400.0);
  // np.hanning(401)[:-1] : 0.5 - 0.5*cos(2*pi*n/(M-1)), M = 401
  for (int n = 0; n < 400; ++n) consts[400 + n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / 400.0));
  std::vector<float> filt;
  compute_mel_filters(m->cfg.n_mels, filt);
  m->lm_mel_pad = ((m->cfg.n_mels + 31) / 32) * 32;
  std::vector<float> filtT((size_t)224 * m->lm_mel_pad, 0.f);
  for (int i = 0; i < m->cfg.n_mels; ++i)
    for (int k = 0; k < 201; ++k) filtT[(size_t)k * m->lm_mel_pad + i] = filt[(size_t)i * 201 + k];
  int rc;
  if ((rc = m->bufs.alloc(&m->lm_consts, 800)) || (rc = m->bufs.alloc(&m->lm_filtT, filtT.size()))) return rc;
  FW_HIP(hipMemcpy(m->lm_consts, consts.data(), 800 * sizeof(float), hipMemcpyHostToDevice));
  FW_HIP(hipMemcpy(m->lm_filtT, filtT.data(), filtT.size() * sizeof(float), hipMemcpyHostToDevice));
  return FW_OK;
}

// ---------------------------------------------------------------- model construction
// live models, for the two ties between them (Model::dependents): a borrowed blob and a joined decoder
static std::mutex g_models_mu;
static std::vector<Model*> g_live_models;

static int alloc_workspaces(Model* m) {
  const fw_config& c = m->cfg;
  const size_t B = m->max_batch, d = c.d_model, T = c.n_audio_ctx;
  m->t_pad = ((c.n_audio_ctx + 63) / 64) * 64;  // 1536
  DevBufs& db = m->bufs;
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  int rc;
  // conv padding rows / V^T time padding must be zero and are never written again: ws_mel_cl, ws_conv1, ws_vt
  if ((rc = db.alloc(&m->ws_offsets, B + 1)) || (rc = db.alloc(&m->ws_chunk_max, B)) || (rc = db.alloc(&m->ws_nframes, B)) ||
      (rc = m->ws_raw.ensure((int64_t)B * c.n_mels * 3008)) || (rc = db.alloc(&m->ws_feat32, B * c.n_mels * 3000)) ||
      (rc = db.zalloc(&m->ws_mel_cl, B * 3002 * m->c_pad)) || (rc = db.zalloc(&m->ws_conv1, B * 3002 * d)) ||
      (rc = db.alloc(&m->ws_x, B * T * d)) || (rc = db.alloc(&m->ws_x2, B * T * d)) || (rc = db.alloc(&m->ws_xn, B * T * d)) ||
      (rc = db.alloc(&m->ws_qk, B * T * 2 * d)) || (rc = db.zalloc(&m->ws_vt, B * d * m->t_pad)) ||
      (rc = db.alloc(&m->ws_att, B * T * d)) || (rc = db.alloc(&m->ws_ffn, B * T * 4 * d)) ||
      (i8 && ((rc = db.alloc(&m->ws_xq.q, B * T * 4 * d)) || (rc = db.alloc(&m->ws_xq.scale, B * T)))))
    return rc;
  if (i8) { m->ws_xq.cap_rows = B * T; m->ws_xq.cap_elems = B * T * 4 * d; }
  return FW_OK;
}

static int model_from_blob(const void* blob_dev, int64_t blob_bytes, bool owned, int device, int max_batch,
                           int max_beam, fw_model** out) {
  FW_CHECK_ARG(max_batch >= 1 && max_batch <= 256, "max_batch must be in [1,256], got %d", max_batch);
  FW_CHECK_ARG(max_beam >= 1 && max_beam <= 16, "max_beam must be in [1,16], got %d", max_beam);
  FW_CHECK_ARG(max_batch * max_beam <= 2048, "max_batch * max_beam must be <= 2048 decoder rows, got %d", max_batch * max_beam);
  FW_CHECK_ARG(blob_bytes >= (int64_t)sizeof(BlobHeader), "weight blob too small");
  BlobHeader h;
  FW_HIP(hipMemcpy(&h, blob_dev, sizeof(h), hipMemcpyDeviceToHost));
  int rc = check_blob_header(h, blob_bytes);
  if (rc) return rc;
  std::vector<BlobEntry> entries(h.n_tensors);
  FW_HIP(hipMemcpy(entries.data(), reinterpret_cast<const char*>(blob_dev) + sizeof(h),
                   entries.size() * sizeof(BlobEntry), hipMemcpyDeviceToHost));
  fw_model* fm = new fw_model();
  Model* m = &fm->impl;
  m->lanes.reserve(kMaxDecodeLanes);   // (lanes[0] stays put while a rebuild appends; other readers: see engine.h)
  m->lanes.emplace_back(new DecodeLane());
  m->cfg = h.cfg;
  m->compute_type = h.compute_type;
  m->device = device;
  m->max_batch = max_batch;
  m->max_beam = max_beam;
  m->blob = const_cast<void*>(blob_dev);
  m->blob_owned = owned;
  m->blob_bytes = blob_bytes;
  m->enc_pool = std::make_shared<EncPool>(m, (size_t)max_batch * h.cfg.n_audio_ctx * h.cfg.d_model);
  auto fail = [&](int code) { fw_model_free(fm); return code; };
  hipError_t he = create_stream(&m->stream, "ENC");
  if (he != hipSuccess) {
    set_error("hipStreamCreate failed: %s", hipGetErrorString(he));
    return fail(FW_ENODEV);
  }
  if ((rc = bind_weights(h, entries.data(), m->blob, *m, &m->has_plain))) return fail(rc);
  m->ln_unfold = env_ln_unfold();   // fp16 evaluation order of the decoder LayerNorms (engine.h)
  if (m->ln_unfold && m->compute_type != FW_COMPUTE_INT8_FLOAT16 && !m->has_plain) {
    set_error("FWAMD_LN_UNFOLD=%d needs a weight blob packed with FWAMD_LN_UNFOLD set (this one carries the folded forms only)",
              m->ln_unfold);
    return fail(FW_EINVAL);
  }
  if ((rc = setup_logmel_consts(m))) return fail(rc);
  if ((rc = alloc_workspaces(m))) return fail(rc);
  m->decode_batch = max_batch;   // the decode workspace itself is created on first use (decoder.hip)
  he = hipDeviceSynchronize();
  if (he != hipSuccess) {
    set_error("device sync after model setup failed: %s", hipGetErrorString(he));
    return fail(FW_ENODEV);
  }
  {
    // a model on a borrowed blob (fw_model_create_from_blob_dev on fw_model_blob's pointer) keeps the owner alive:
    // fw_model_free(owner) is deferred until its last dependent is gone
    std::lock_guard<std::mutex> lk(g_models_mu);
    if (!owned)
      for (Model* o : g_live_models)
        if (o->blob == m->blob && o->blob_owned) { m->blob_owner = o; o->dependents += 1; break; }
    g_live_models.push_back(m);
  }
  m->self = fm;
  *out = fm;
  return FW_OK;
}

// CU mask of n CUs (a multiple of 32), the same number in every XCD.  Whether bit i of a HIP CU mask is CU (i / 8) of XCD
// (i % 8) — the order the KFD documents for multi-XCC parts — or CU (i % 32) of XCD (i / 32) does not matter here: with
// a = i % 8, b = i / 8 the rule (a + b) % 8 < n / 32 selects n / 8 CUs of every XCD under either reading (for a fixed a the
// 32 values of b hit every residue four times; for the four b of one XCD of the second reading every a-residue once each).
// invert: the complement (256 - n CUs, exactly the ones the plain mask leaves out) — the two sides of a partition.
static void balanced_cu_mask(int n_cus, bool invert, uint32_t mask[8]) {
  const int k = n_cus / 32;
  for (int w = 0; w < 8; ++w) mask[w] = 0;
  for (int i = 0; i < 256; ++i) {
    const bool in = ((i % 8) + (i / 8)) % 8 < k;
    if (in != invert) mask[i >> 5] |= 1u << (i & 31);
  }
}

// role "ENC" (a worker's encoder stream) or "DEC" (a decode lane's streams).  Environment, read per stream creation:
//   FWAMD_<role>_STREAM_PRIO = high | low       stream priority (measured: no effect, profiles/r05_ab_stream_priority.jsonl)
//   FWAMD_<role>_CUS = n | -n                   CU-masked stream: n CUs (multiple of 32, the same share of every XCD), or
//                                               with a minus sign the 256 - n CUs the mask of n leaves out — so
//                                               FWAMD_DEC_CUS=96 FWAMD_ENC_CUS=-96 is a disjoint 96 / 160 partition
//                                               (profiles/r06_ab_overlap.jsonl).  CU-mask streams are BLOCKING streams: the
//                                               hot path issues nothing on the default stream (results are copied on the decode stream), only set-up copies wait.
hipError_t create_stream(hipStream_t* st, const char* role) {
  char name[64];
  snprintf(name, sizeof(name), "FWAMD_%s_CUS", role);
  if (const char* c = getenv(name)) {
    const int v = atoi(c), n = v < 0 ? -v : v;
    if (n >= 32 && n <= 224 && n % 32 == 0) {
      uint32_t mask[8];
      balanced_cu_mask(n, v < 0, mask);
      return hipExtStreamCreateWithCUMask(st, 8, mask);
    }
  }
  snprintf(name, sizeof(name), "FWAMD_%s_STREAM_PRIO", role);
  const char* e = getenv(name);
  if (e && (!strcmp(e, "high") || !strcmp(e, "low"))) {
    int least = 0, greatest = 0;   // numerically: greatest priority <= least priority
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
      return hipStreamCreateWithPriority(st, hipStreamNonBlocking, e[0] == 'h' ? greatest : least);
  }
  return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

// ---------------------------------------------------------------- layers
fwk::GemmParams gemm_params(const LinearW& L, const LinCall& c, int64_t ldw) {
  fwk::GemmParams p{};
  if (const QuantRows* xq = c.in.xq) {   // int8 x int8 -> int32 MFMA, de-quantising epilogue: codes where the halves were
    p.A = reinterpret_cast<const half_t*>(xq->q); p.lda = xq->ld; p.a_bstride = c.M * xq->ld;
    p.W = reinterpret_cast<const half_t*>(L.wq);
    p.a_scale = xq->scale; p.as_bstride = c.M; p.w_scale = L.wscale;
  } else {
    p.A = c.in.A; p.lda = c.in.lda; p.a_bstride = c.in.a_bs;
    p.W = L.w;
  }
  p.ldw = ldw;
  p.bias = L.b;
  p.res = c.res; p.ldr = c.ldr; p.r_bstride = c.r_bs;
  p.C = c.C; p.ldc = c.ldc; p.c_bstride = c.c_bs;
  p.M = c.M; p.N = L.N; p.K = L.K;
  p.act = c.act;
  p.head_rows = c.head_rows;
  p.n_layers = c.n_layers; p.w_lstride = c.w_ls; p.bias_lstride = c.b_ls; p.c_lstride = c.c_ls;
  return p;
}

int run_linear(Model* m, const LinearW& L, const LinCall& c) {
  if (const QuantRows* xq = c.in.xq)
    FW_CHECK_ARG(xq->scale && xq->rows == (int64_t)c.batch * c.M && xq->ld == L.K,
                 "int8 gemm: the quantised input holds %lld rows of %lld, the call reads %lld rows of %d", (long long)xq->rows,
                 (long long)xq->ld, (long long)c.batch * c.M, L.K);
  if (fwk::launch_gemm(c.st ? c.st : m->stream, gemm_params(L, c, L.K), c.batch, c.trans) != 0) {
    set_error("%sgemm: unsupported shape M=%d N=%d K=%d lda=%lld layers=%d", c.in.xq ? "int8 " : "", c.M, L.N, L.K,
              (long long)c.in.lda, c.n_layers);
    return FW_ERUNTIME;
  }
  return FW_OK;
}

int quantise_rows(Model* m, const half_t* A, const LNW* ln, int64_t rows, int K, hipStream_t st, QuantRows& qr) {
  FW_CHECK_ARG(qr.fits(rows, K), "quantise_rows: %lld rows x %d = %lld elements, the buffer holds %lld rows, %lld elements",
               (long long)rows, K, (long long)(rows * K), (long long)qr.cap_rows, (long long)qr.cap_elems);
  fwk::launch_quant_rows(st ? st : m->stream, A, K, ln ? ln->g : nullptr, ln ? ln->b : nullptr, qr.q, qr.scale, (int)rows, K);
  qr.rows = rows; qr.ld = K;
  return FW_OK;
}

int run_encoder(Model* m, int B, half_t* out) {
  const fw_config& c = m->cfg;
  const int d = c.d_model, T = c.n_audio_ctx, H = c.n_heads;
  const int64_t xs = (int64_t)T * d, vts = (int64_t)d * m->t_pad;
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  auto gemm_flops = [&](double rows, double k) { return 2.0 * B * rows * d * k; };
  int rc;
  {
    // conv1: k=3, s=1 over the channel-last mel image; GELU; output rows 1..3000 of the padded conv1 image
    ProfScope ps(m, PF_ENC_GEMM, gemm_flops(3000.0, 3.0 * c.n_mels), 0);
    if ((rc = run_linear(m, m->conv1, {.in = {m->ws_mel_cl, m->c_pad, (int64_t)3002 * m->c_pad}, .C = m->ws_conv1 + d,
                                       .ldc = d, .c_bs = (int64_t)3002 * d, .M = 3000, .batch = B, .act = 1})))
      return rc;
  }
  {
    // conv2: k=3, s=2: row t reads padded rows 2t..2t+2 (lda = 2d, K = 3d); GELU; + positional embedding
    ProfScope ps(m, PF_ENC_GEMM, gemm_flops(T, 3.0 * d), 0);
    if ((rc = run_linear(m, m->conv2, {.in = {m->ws_conv1, 2 * d, (int64_t)3002 * d}, .C = m->ws_x, .ldc = d, .c_bs = xs,
                                       .res = m->enc_pos, .ldr = d, .r_bs = 0, .M = T, .batch = B, .act = 1})))
      return rc;
  }
  half_t* x = m->ws_x;
  half_t* x2 = m->ws_x2;
  // The two compute types meet in the input of a layer's linears, a [B * T][K] dense, through LayerNorm ln when given:
  // fp16 launches the LayerNorm into ws_xn (normed, before the GEMMs' scope opens) and reads halves; int8_float16
  // quantises every linear's input per row, the LayerNorm fused into the quantiser (input, inside the GEMMs' scope)
  auto normed = [&](const half_t* a, const LNW& ln) -> const half_t* {
    if (i8) return a;
    ProfScope ps(m, PF_ENC_LN, 0, 4.0 * B * T * d);
    fwk::launch_layernorm(m->stream, a, ln.g, ln.b, m->ws_xn, B * T, d);
    return m->ws_xn;
  };
  auto input = [&](const half_t* a, int K, const LNW* ln, LinIn& in) -> int {
    if (!i8) { in = {a, K, (int64_t)T * K}; return FW_OK; }
    in = {.xq = &m->ws_xq};
    return quantise_rows(m, a, ln, (int64_t)B * T, K, m->stream, m->ws_xq);
  };
  for (int l = 0; l < c.n_enc_layers; ++l) {
    const EncLayerW& L = m->enc[l];
    LinIn in;
    const half_t* h = normed(x, L.ln1);
    {
      ProfScope ps(m, PF_ENC_GEMM, gemm_flops(T, 3.0 * d), 0);
      if ((rc = input(h, d, &L.ln1, in)) ||   // (int8_float16: quantised once, projected twice)
          (rc = run_linear(m, L.qk, {.in = in, .C = m->ws_qk, .ldc = 2 * d, .c_bs = 2 * xs, .M = T, .batch = B})) ||
          (rc = run_linear(m, L.v, {.in = in, .C = m->ws_vt, .ldc = m->t_pad, .c_bs = vts, .M = T, .batch = B, .trans = true})))
        return rc;
    }
    {
      ProfScope ps(m, PF_ENC_ATTN, 4.0 * B * (double)T * T * d, 0);
      fwk::launch_attn_enc(m->stream, {.q = m->ws_qk, .k = m->ws_qk + d, .ld = 2 * d, .qk_bstride = 2 * xs, .vt = m->ws_vt,
                                       .ldvt = m->t_pad, .vt_bstride = vts, .out = m->ws_att, .ldo = d, .o_bstride = xs,
                                       .B = B, .H = H, .T = T});
    }
    // the profile's grouping: int8_float16 has ONE scope over the out-projection and the FFN (9 d); fp16 closes the
    // out-projection's (d) for the LayerNorm's own scope and opens the FFN's (8 d) after it
    std::optional<ProfScope> ps;
    ps.emplace(m, PF_ENC_GEMM, gemm_flops(T, i8 ? 9.0 * d : d), 0);
    if ((rc = input(m->ws_att, d, nullptr, in)) ||
        (rc = run_linear(m, L.out, {.in = in, .C = x2, .ldc = d, .c_bs = xs, .res = x, .ldr = d, .r_bs = xs, .M = T, .batch = B})))
      return rc;
    if (!i8) ps.reset();
    h = normed(x2, L.ln2);
    if (!i8) ps.emplace(m, PF_ENC_GEMM, gemm_flops(T, 8.0 * d), 0);
    if ((rc = input(h, d, &L.ln2, in)) ||
        (rc = run_linear(m, L.ffn1, {.in = in, .C = m->ws_ffn, .ldc = 4 * d, .c_bs = 4 * xs, .M = T, .batch = B, .act = 1})) ||
        (rc = input(m->ws_ffn, 4 * d, nullptr, in)) ||
        (rc = run_linear(m, L.ffn2, {.in = in, .C = x, .ldc = d, .c_bs = xs, .res = x2, .ldr = d, .r_bs = xs, .M = T, .batch = B})))
      return rc;
  }
  {
    ProfScope ps(m, PF_ENC_LN, 0, 4.0 * B * T * d);
    fwk::launch_layernorm(m->stream, x, m->enc_ln_post.g, m->enc_ln_post.b, out, B * T, d);
  }
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) {
    set_error("encoder launch failed: %s", hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  return FW_OK;
}

int EncPool::take(half_t** p) {
  {
    std::lock_guard<std::mutex> lk(mu);
    if (!free.empty()) {
      *p = free.back();
      free.pop_back();
      return FW_OK;
    }
  }
  return dev_alloc_t(p, elems);
}
void EncPool::give(half_t* p) {
  std::unique_lock<std::mutex> lk(mu);
  if (!closed) { free.push_back(p); return; }
  lk.unlock();
  (void)hipFree(p);
}
void EncPool::close() {   // fw_model_free: the tensors still out release their buffers themselves
  std::vector<half_t*> rest;
  {
    std::lock_guard<std::mutex> lk(mu);
    closed = true;
    model.store(nullptr);
    rest.swap(free);
  }
  for (half_t* p : rest) (void)hipFree(p);
}

static int new_tensor(Model* m, int B, fw_tensor** out) {
  fw_tensor* t = new fw_tensor();
  t->impl.pool = m->enc_pool;
  t->impl.B = B;
  t->impl.T = m->cfg.n_audio_ctx;
  t->impl.D = m->cfg.d_model;
  t->impl.id = next_tensor_id();
  if (int rc = m->enc_pool->take(&t->impl.data)) {
    delete t;
    return rc;
  }
  *out = t;
  return FW_OK;
}

// the shared tail of the encode entry points: the encoder on the mel image in ws_mel_cl, into a new tensor
static int encode_to_tensor(Model* m, int B, const char* what, fw_tensor** out) {
  fw_tensor* t = nullptr;
  int rc = new_tensor(m, B, &t);
  if (rc) return rc;
  if ((rc = run_encoder(m, B, t->impl.data))) {
    fw_tensor_free(t);
    return rc;
  }
  hipError_t he = hipStreamSynchronize(m->stream);
  if (he != hipSuccess) {
    fw_tensor_free(t);
    set_error("%s failed: %s", what, hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  prof_collect(m->prof);
  *out = t;
  return FW_OK;
}

static int check_offsets(const int64_t* offsets, int B, int64_t* total, int* max_frames) {
  FW_CHECK_ARG(offsets && offsets[0] == 0, "offsets[0] must be 0");
  int mf = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = offsets[b + 1] - offsets[b];
    FW_CHECK_ARG(n >= 0 && n < (int64_t)1 << 30, "chunk %d has invalid length %lld", b, (long long)n);
    mf = std::max(mf, (int)((n + 160) / 160));
  }
  *total = offsets[B];
  *max_frames = mf;
  return FW_OK;
}

// log-mel for B ragged chunks whose PCM already sits at pcm_dev; writes ws_feat32 and/or ws_mel_cl
static int logmel_batch(Model* m, const float* pcm_dev, const int64_t* offsets_host, int B, bool want_f32,
                        bool want_cl) {
  int64_t total;
  int max_frames;
  int rc = check_offsets(offsets_host, B, &total, &max_frames);
  if (rc) return rc;
  const int stride = std::max(3008, (max_frames + 7) / 8 * 8);
  if ((rc = m->ws_raw.ensure((int64_t)B * m->cfg.n_mels * stride))) return rc;
  FW_HIP(hipMemcpyAsync(m->ws_offsets, offsets_host, (B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, m->stream));
  {
    ProfScope ps(m, PF_LOGMEL, 0, (double)total * 4 + (double)B * m->cfg.n_mels * 3000 * (want_f32 ? 4 : 2));
    fwk::launch_logmel(m->stream, pcm_dev, m->ws_offsets, B, max_frames, m->lm_consts, m->lm_filtT, m->lm_mel_pad,
                       m->cfg.n_mels, m->ws_raw.p, (int64_t)m->cfg.n_mels * stride, stride, m->ws_chunk_max, 1, 3000,
                       want_f32 ? m->ws_feat32 : nullptr, want_cl ? m->ws_mel_cl : nullptr, m->c_pad, m->ws_nframes);
  }
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) {
    set_error("logmel launch failed: %s", hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  return FW_OK;
}

}  // namespace fw

using namespace fw;

// ================================================================== C ABI
extern "C" {

const char* fw_last_error(void) { return g_err; }
int32_t fw_abi_version(void) { return FW_ABI_VERSION; }

int32_t fw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t fw_model_create(const fw_config* cfg, const fw_weight* weights, int32_t n_weights, int32_t compute_type,
                        int32_t device_index, int32_t max_batch, int32_t max_beam, fw_model** out) {
  FW_CHECK_ARG(cfg && weights && out, "null argument");
  FW_CHECK_ARG(compute_type == FW_COMPUTE_FLOAT16 || compute_type == FW_COMPUTE_INT8_FLOAT16,
               "unsupported compute_type %d", compute_type);
  int rc = check_config(cfg);
  if (rc) return rc;
  const int ndev = fw_device_count();
  if (ndev <= 0) {
    set_error("no HIP device visible: libfwamd has no CPU fallback");
    return FW_ENODEV;
  }
  FW_CHECK_ARG(device_index >= 0 && device_index < ndev, "device_index %d out of range (%d devices)", device_index,
               ndev);
  FW_HIP(hipSetDevice(device_index));
  std::vector<uint8_t> blob;
  if ((rc = pack_blob(cfg, weights, n_weights, compute_type, blob))) return rc;
  void* dblob = nullptr;
  if ((rc = dev_alloc(&dblob, blob.size()))) return rc;
  hipError_t he = hipMemcpy(dblob, blob.data(), blob.size(), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    (void)hipFree(dblob);
    set_error("weight upload failed: %s", hipGetErrorString(he));
    return FW_ENODEV;
  }
  rc = model_from_blob(dblob, (int64_t)blob.size(), true, device_index, max_batch, max_beam, out);
  return rc;
}

int32_t fw_pack_blob_size(const fw_config* cfg, const fw_weight* weights, int32_t n_weights, int32_t compute_type,
                          int64_t* size_out, void** handle_out) {
  FW_CHECK_ARG(cfg && weights && size_out && handle_out, "null argument");
  int rc = check_config(cfg);
  if (rc) return rc;
  auto* blob = new std::vector<uint8_t>();
  if ((rc = pack_blob(cfg, weights, n_weights, compute_type, *blob))) {
    delete blob;
    return rc;
  }
  *size_out = (int64_t)blob->size();
  *handle_out = blob;
  return FW_OK;
}
int32_t fw_pack_blob_copy(void* handle, void* dst, int64_t dst_bytes) {
  auto* blob = reinterpret_cast<std::vector<uint8_t>*>(handle);
  FW_CHECK_ARG(blob && dst && dst_bytes >= (int64_t)blob->size(), "bad blob copy arguments");
  memcpy(dst, blob->data(), blob->size());
  return FW_OK;
}
void fw_pack_blob_free(void* handle) { delete reinterpret_cast<std::vector<uint8_t>*>(handle); }

int32_t fw_model_create_from_blob_dev(const fw_config* cfg, const void* blob_dev, int64_t blob_bytes,
                                      int32_t compute_type, int32_t device_index, int32_t max_batch,
                                      int32_t max_beam, fw_model** out) {
  (void)cfg;
  (void)compute_type;
  FW_CHECK_ARG(blob_dev && out, "null argument");
  const int ndev = fw_device_count();
  if (ndev <= 0) {
    set_error("no HIP device visible: libfwamd has no CPU fallback");
    return FW_ENODEV;
  }
  FW_CHECK_ARG(device_index >= 0 && device_index < ndev, "device_index %d out of range", device_index);
  FW_HIP(hipSetDevice(device_index));
  return model_from_blob(blob_dev, blob_bytes, false, device_index, max_batch, max_beam, out);
}

void fw_model_free(fw_model* fm) {
  if (!fm) return;
  Model* m = &fm->impl;
  Model* release[2] = {nullptr, nullptr};
  {
    std::lock_guard<std::mutex> lk(g_models_mu);
    if (m->dependents > 0) {   // workers still use this model's weights / decode workspace: freed with the last one
      m->free_deferred = true;
      return;
    }
    g_live_models.erase(std::remove(g_live_models.begin(), g_live_models.end(), m), g_live_models.end());
    release[0] = m->blob_owner;
    release[1] = m->decoder;
  }
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  m->lanes.clear();         // (each waits for its stream first)
  cross_pool_free(m);
  m->enc_pool->close();
  if (m->blob && m->blob_owned) (void)hipFree(m->blob);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete fm;   // (the workspaces go with it: Model::bufs, ws_pcm, ws_raw)
  for (Model* t : release) {
    if (!t) continue;
    bool free_now = false;
    {
      std::lock_guard<std::mutex> lk(g_models_mu);
      t->dependents -= 1;
      free_now = t->free_deferred && t->dependents == 0;
    }
    if (free_now) fw_model_free(static_cast<fw_model*>(t->self));
  }
}

int32_t fw_model_blob(const fw_model* fm, void** blob_dev, int64_t* blob_bytes) {
  FW_CHECK_ARG(fm && blob_dev && blob_bytes, "null argument");
  *blob_dev = fm->impl.blob;
  *blob_bytes = fm->impl.blob_bytes;
  return FW_OK;
}

int32_t fw_model_info(const fw_model* fm, fw_config* cfg_out, int32_t* compute_type, int32_t* device_index,
                      int32_t* max_batch, int32_t* max_beam) {
  FW_CHECK_ARG(fm, "null model");
  const Model* m = &fm->impl;
  if (cfg_out) *cfg_out = m->cfg;
  if (compute_type) *compute_type = m->compute_type;
  if (device_index) *device_index = m->device;
  if (max_batch) *max_batch = m->max_batch;
  if (max_beam) *max_beam = m->max_beam;
  return FW_OK;
}

// rows of the largest decode run of a group (decoder.hip: DEC_RUN_MAX_ROWS)
#define DEC_GROUP_RUN_ROWS 1600
// lanes a decode group builds once it holds four encoder batches: two, or FWAMD_DECODE_LANES (1 .. kMaxDecodeLanes)
static int env_decode_lanes() {
  const char* e = getenv("FWAMD_DECODE_LANES");
  return e ? std::min(kMaxDecodeLanes, std::max(1, atoi(e))) : 2;
}

int32_t fw_model_set_decode_batch(fw_model* fm, int32_t decode_batch) {
  FW_CHECK_ARG(fm, "null model");
  Model* m = &fm->impl;
  FW_CHECK_ARG(!m->decoder, "this model has joined another model's decoder");
  FW_CHECK_ARG(decode_batch >= 1, "decode_batch must be positive");
  {
    // The workspaces, the pool and the lanes are rebuilt below: not while the group has work, and no fw_generate
    // call may read capacities / dm->lanes or queue a request until the rebuild is done (grp.resizing: callers wait
    // on grp.cv).  fw_detect_language / fw_align hold the mutex of lanes[0], which the rebuild takes.
    std::lock_guard<std::mutex> gl(m->grp.mu);
    FW_CHECK_ARG(m->grp.active_runs == 0 && !m->grp.gathering && m->grp.queue.empty() && !m->grp.resizing,
                 "decode runs are queued or in flight: set the decode batch before the first generate call or after the last one returned");
    m->grp.resizing = true;
  }
  struct Done {   // whatever the outcome: let the callers in again
    DecodeGroup& g;
    ~Done() {
      { std::lock_guard<std::mutex> gl(g.mu); g.resizing = false; }
      g.cv.notify_all();
    }
  } done{m->grp};
  DecodeLane* lane0 = m->lanes[0].get();   // (stays through the rebuild: its mutex is held)
  std::lock_guard<std::mutex> lk(lane0->mu);
  FW_HIP(hipSetDevice(m->device));
  // Sizes, in 70 % of the free HBM:
  //   pool   = the cross-attention K / V^T of `decode_batch` chunks (whole encoder batches, at least one): what the
  //            workers of the group keep in flight, ONE copy whatever the number of lanes;
  //   lanes  = two (two concurrent decode runs: DecodeLane) when the group holds at least four encoder batches,
  //            each with a workspace for the largest run there can be: the pool's chunks, at most DEC_GROUP_RUN_ROWS rows
  //            (decoder.hip caps runs there; one lane: 2048 rows).  The self-attention cache of a lane is rows x
  //            positions and a RUN lays it out for its own max_length, so when the budget is short the positions per
  //            row are lowered first (down to 160: a run that asks for more simply holds fewer rows), then the pool.
  int want = std::max(decode_batch, m->max_batch) / m->max_batch * m->max_batch;
  const int n_lanes = want >= 4 * m->max_batch ? env_decode_lanes() : 1;
  const int max_rows = n_lanes >= 2 ? DEC_GROUP_RUN_ROWS : 2048;
  auto lane_of = [&](int pool_chunks) {
    int lc = pool_chunks;
    while (lc > m->max_batch && (int64_t)lc * m->max_beam > max_rows) lc -= m->max_batch;
    return lc;
  };
  size_t free_b = 0, total_b = 0;
  FW_HIP(hipMemGetInfo(&free_b, &total_b));
  for (const auto& l : m->lanes)
    if (l->gen) free_b += (size_t)gen_workspace_bytes(m, lane_chunks_of(m), m->decode_self_ctx);
  if (m->xpool) free_b += (size_t)cross_pool_bytes(m, std::max(m->decode_batch, m->max_batch));
  const int64_t budget = (int64_t)(0.7 * (double)free_b);
  const int NT = m->cfg.n_text_ctx;
  const int ctx_steps[] = {NT, 320, 224, 160};
  int self_ctx = NT;
  for (;;) {
    bool fits = false;
    for (int cs : ctx_steps) {
      if (cs > NT) continue;
      if (cross_pool_bytes(m, want) + n_lanes * gen_workspace_bytes(m, lane_of(want), cs) <= budget) { self_ctx = cs; fits = true; break; }
    }
    if (fits || want <= m->max_batch) break;
    want -= m->max_batch;
  }
  const int lane_batch = lane_of(want);
  const bool lanes_ok = n_lanes == (int)m->lanes.size();
  if (lane0->gen && m->xpool && lanes_ok && want == m->decode_batch && lane_batch == lane_chunks_of(m) &&
      self_ctx == m->decode_self_ctx)
    return FW_OK;
  if (lane0->stream) FW_HIP(hipStreamSynchronize(lane0->stream));
  // The old state goes first (its HBM is in the budget): the group is as fw_model_create made it, one lane without a
  // workspace, no pool, one encoder batch.  All is then built at the new sizes and committed together, or reset again.
  auto reset = [&] {
    m->lanes.resize(1);
    gen_workspace_free(lane0);
    cross_pool_free(m);
    m->decode_batch = m->max_batch; m->lane_batch = 0; m->decode_self_ctx = 0;
  };
  reset();
  std::vector<std::unique_ptr<DecodeLane>> further;   // lanes 1 .. n_lanes - 1 (freed with the vector on failure)
  int rc = cross_pool_ensure(m, want);
  if (!rc) rc = gen_workspace_build(m, lane0, lane_batch, self_ctx);
  for (int k = 1; !rc && k < n_lanes; ++k) {
    further.emplace_back(new DecodeLane());
    further.back()->prof.on = m->prof.on;
    // Nothing launches on `spare`, but without it four lanes lose 4.5 % (bench --decode-lanes 4, FWAMD_DECODE_LANES=4,
    // alternating: with 3 136 3 230 3 220 3 217x, without 3 010 3 083 3 079 3 068x; two lanes: the same)
    const hipError_t he = create_stream(&further.back()->spare, "DEC");
    if (he != hipSuccess) set_error("hipStreamCreate failed: %s", hipGetErrorString(he));
    rc = he != hipSuccess ? FW_ENODEV : gen_workspace_build(m, further.back().get(), lane_batch, self_ctx);
  }
  if (rc) { reset(); return rc; }
  m->decode_batch = want; m->lane_batch = lane_batch; m->decode_self_ctx = self_ctx;
  for (auto& l : further) m->lanes.push_back(std::move(l));
  return FW_OK;
}

int32_t fw_model_set_decode_lanes(fw_model* fm, int32_t lanes) {
  FW_CHECK_ARG(fm, "null model");
  Model* dm = decoder_of(&fm->impl);
  int have;
  {
    std::lock_guard<std::mutex> gl(dm->grp.mu);     // (the lanes are rebuilt under grp.resizing)
    // (a group that has not built its further lanes yet still takes 2, or what it will build)
    have = std::max({2, env_decode_lanes(), (int)dm->lanes.size()});
  }
  FW_CHECK_ARG(lanes >= 1 && lanes <= have, "decode lanes: 1 .. %d", have);
  dm->grp.lanes_enabled.store(lanes);
  return FW_OK;
}

int32_t fw_model_set_merge_wait(fw_model* fm, int32_t wait_ms, int32_t fill_percent) {
  FW_CHECK_ARG(fm, "null model");
  FW_CHECK_ARG(wait_ms >= -1 && wait_ms <= 10000, "merge wait: -1 (one encoder pass), 0 (never) or milliseconds <= 10000");
  FW_CHECK_ARG(fill_percent >= 1 && fill_percent <= 100, "merge fill: 1 .. 100 percent of a run's chunk capacity");
  DecodeGroup& g = decoder_of(&fm->impl)->grp;
  g.merge_wait_ms.store(wait_ms);
  g.merge_fill_pct.store(fill_percent);
  return FW_OK;
}

int32_t fw_model_decode_batch(const fw_model* fm) {
  if (!fm) return 0;
  const Model* m = decoder_of(&fm->impl);
  return std::max(m->decode_batch, m->max_batch);
}

int32_t fw_model_run_capacity(const fw_model* fm) {
  if (!fm) return 0;
  return lane_chunks_of(decoder_of(&fm->impl));
}

int32_t fw_model_decode_stats(const fw_model* fm, int64_t* runs, int64_t* requests, int64_t* chunks,
                              int32_t* max_run_chunks) {
  FW_CHECK_ARG(fm, "null model");
  const Model* m = decoder_of(&fm->impl);
  if (runs) *runs = m->grp.n_runs.load();
  if (requests) *requests = m->grp.n_requests.load();
  if (chunks) *chunks = m->grp.n_chunks.load();
  if (max_run_chunks) *max_run_chunks = m->grp.max_run_chunks.load();
  return FW_OK;
}

int32_t fw_model_join_decoder(fw_model* fm, fw_model* decoder) {
  FW_CHECK_ARG(fm && decoder && fm != decoder, "need two distinct models");
  Model* m = &fm->impl;
  Model* d = &decoder->impl;
  FW_CHECK_ARG(!d->decoder, "the decoder model has itself joined another decoder");
  FW_CHECK_ARG(m->device == d->device && m->blob == d->blob && m->max_batch == d->max_batch && m->max_beam == d->max_beam,
               "models that share a decoder must share device, weight blob, max_batch and max_beam");
  FW_CHECK_ARG(!m->decoder, "this model has already joined a decoder");
  DecodeLane* lane = m->lanes[0].get();
  std::lock_guard<std::mutex> lk(lane->mu);
  FW_HIP(hipSetDevice(m->device));
  if (lane->stream) FW_HIP(hipStreamSynchronize(lane->stream));
  gen_workspace_free(lane);
  cross_pool_free(m);
  {
    std::lock_guard<std::mutex> lk2(g_models_mu);   // the primary outlives its workers (fw_model_free defers)
    d->dependents += 1;
  }
  m->decoder = d;
  return FW_OK;
}

int32_t fw_logmel(fw_model* fm, const float* pcm, const int64_t* offsets, int32_t B, float* out,
                  int32_t* n_frames_out) {
  FW_CHECK_ARG(fm && offsets && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  int64_t total; int mf;
  int rc = check_offsets(offsets, B, &total, &mf);
  if (rc) return rc;
  FW_CHECK_ARG(total == 0 || pcm, "null pcm");
  if ((rc = m->ws_pcm.ensure(std::max<int64_t>(total, 1)))) return rc;
  if (total) FW_HIP(hipMemcpyAsync(m->ws_pcm.p, pcm, total * sizeof(float), hipMemcpyHostToDevice, m->stream));
  if ((rc = logmel_batch(m, m->ws_pcm.p, offsets, B, true, false))) return rc;
  FW_HIP(hipMemcpyAsync(out, m->ws_feat32, (size_t)B * m->cfg.n_mels * 3000 * sizeof(float), hipMemcpyDeviceToHost,
                        m->stream));
  if (n_frames_out)
    FW_HIP(hipMemcpyAsync(n_frames_out, m->ws_nframes, B * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  FW_HIP(hipStreamSynchronize(m->stream));
  return FW_OK;
}

int32_t fw_logmel_full(fw_model* fm, const float* pcm, int64_t n_samples, float* out, int64_t out_frames) {
  FW_CHECK_ARG(fm && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(n_samples >= 0 && n_samples < (int64_t)1 << 30, "invalid n_samples");
  const int64_t nf = (n_samples + 160) / 160;
  FW_CHECK_ARG(out_frames == nf, "out_frames must be n_samples/160 + 1 = %lld, got %lld", (long long)nf,
               (long long)out_frames);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  int rc;
  if ((rc = m->ws_pcm.ensure(std::max<int64_t>(n_samples, 1)))) return rc;
  if (n_samples) FW_HIP(hipMemcpyAsync(m->ws_pcm.p, pcm, n_samples * sizeof(float), hipMemcpyHostToDevice, m->stream));
  const int stride = (int)((nf + 7) / 8 * 8);
  if ((rc = m->ws_raw.ensure((int64_t)m->cfg.n_mels * std::max(stride, 3008)))) return rc;
  const int rstride = std::max(stride, 3008);
  int64_t offs[2] = {0, n_samples};
  FW_HIP(hipMemcpyAsync(m->ws_offsets, offs, 2 * sizeof(int64_t), hipMemcpyHostToDevice, m->stream));
  float* dout = nullptr;
  if ((rc = dev_alloc_t(&dout, (size_t)m->cfg.n_mels * nf))) return rc;
  {
    ProfScope ps(m, PF_LOGMEL, 0, (double)n_samples * 4 + (double)m->cfg.n_mels * nf * 4);
    fwk::launch_logmel(m->stream, m->ws_pcm.p, m->ws_offsets, 1, (int)nf, m->lm_consts, m->lm_filtT, m->lm_mel_pad,
                       m->cfg.n_mels, m->ws_raw.p, (int64_t)m->cfg.n_mels * rstride, rstride, m->ws_chunk_max, 0,
                       (int)nf, dout, nullptr, m->c_pad, nullptr);
  }
  hipError_t he = hipMemcpyAsync(out, dout, (size_t)m->cfg.n_mels * nf * sizeof(float), hipMemcpyDeviceToHost,
                                 m->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(m->stream);
  (void)hipFree(dout);
  if (he != hipSuccess) {
    set_error("logmel_full failed: %s", hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  return FW_OK;
}

namespace {
// tells the device's decode group that a request is on its way (the leader of the next decode run waits a moment
// for it instead of starting with a nearly empty workspace)
struct EncodingMark {
  fw::DecodeGroup& g;
  std::chrono::steady_clock::time_point t0;
  explicit EncodingMark(fw::Model* m) : g(fw::decoder_of(m)->grp) {
    g.encoding.fetch_add(1);
    // One encoder pass at a time per device: a pass fills the chip by itself, several at once only time-slice
    // (measured +1.5 % throughput with the lock, and per-kernel event timings stay meaningful).  The decode run of
    // the group keeps going on its own stream next to it.
    g.enc_mu.lock();
    t0 = std::chrono::steady_clock::now();
  }
  ~EncodingMark() {
    const int us = (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    const int old = g.enc_pass_us.load();
    g.enc_pass_us.store(old ? (3 * old + us) / 4 : us);
    g.enc_mu.unlock();
    g.encoding.fetch_sub(1);
    g.cv.notify_all();
  }
};
}  // namespace

int32_t fw_encode(fw_model* fm, const float* features, int32_t B, fw_tensor** out) {
  FW_CHECK_ARG(fm && features && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  EncodingMark mark(m);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  FW_HIP(hipMemcpyAsync(m->ws_feat32, features, (size_t)B * m->cfg.n_mels * 3000 * sizeof(float),
                        hipMemcpyHostToDevice, m->stream));
  fwk::launch_features_to_cl(m->stream, m->ws_feat32, B, m->cfg.n_mels, 3000, m->ws_mel_cl, m->c_pad);
  return encode_to_tensor(m, B, "encode", out);
}

static int encode_pcm_common(Model* m, const float* pcm_dev, const int64_t* offsets, int B, fw_tensor** out) {
  if (int rc = logmel_batch(m, pcm_dev, offsets, B, false, true)) return rc;
  return encode_to_tensor(m, B, "encode_pcm", out);
}

int32_t fw_encode_pcm(fw_model* fm, const float* pcm, const int64_t* offsets, int32_t B, fw_tensor** out) {
  FW_CHECK_ARG(fm && offsets && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  EncodingMark mark(m);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  int64_t total; int mf;
  int rc = check_offsets(offsets, B, &total, &mf);
  if (rc) return rc;
  FW_CHECK_ARG(total == 0 || pcm, "null pcm");
  if ((rc = m->ws_pcm.ensure(std::max<int64_t>(total, 1)))) return rc;
  if (total) FW_HIP(hipMemcpyAsync(m->ws_pcm.p, pcm, total * sizeof(float), hipMemcpyHostToDevice, m->stream));
  return encode_pcm_common(m, m->ws_pcm.p, offsets, B, out);
}

int32_t fw_encode_pcm_dev(fw_model* fm, const float* pcm_dev, const int64_t* offsets, int32_t B, fw_tensor** out) {
  FW_CHECK_ARG(fm && pcm_dev && offsets && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  EncodingMark mark(m);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  return encode_pcm_common(m, pcm_dev, offsets, B, out);
}

int32_t fw_tensor_shape(const fw_tensor* t, int32_t* B, int32_t* T, int32_t* D) {
  FW_CHECK_ARG(t, "null tensor");
  if (B) *B = t->impl.B;
  if (T) *T = t->impl.T;
  if (D) *D = t->impl.D;
  return FW_OK;
}

int32_t fw_tensor_to_host(fw_model* fm, const fw_tensor* t, float* out) {
  FW_CHECK_ARG(fm && t && out, "null argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const size_t n = (size_t)t->impl.B * t->impl.T * t->impl.D;
  DevBufs db;
  float* tmp = nullptr;
  if (int rc = db.alloc(&tmp, n)) return rc;
  fwk::launch_f16_to_f32(m->stream, t->impl.data, tmp, (int64_t)n);
  hipError_t he = hipMemcpyAsync(out, tmp, n * sizeof(float), hipMemcpyDeviceToHost, m->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(m->stream);
  if (he != hipSuccess) {
    set_error("tensor_to_host failed: %s", hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  return FW_OK;
}

int32_t fw_tensor_from_host(fw_model* fm, const float* data, int32_t B, fw_tensor** out) {
  FW_CHECK_ARG(fm && data && out, "null argument");
  Model* m = &fm->impl;
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  fw_tensor* t = nullptr;
  int rc = new_tensor(m, B, &t);
  if (rc) return rc;
  const size_t n = (size_t)B * t->impl.T * t->impl.D;
  DevBufs db;
  float* tmp = nullptr;
  if ((rc = db.alloc(&tmp, n))) { fw_tensor_free(t); return rc; }
  hipError_t he = hipMemcpyAsync(tmp, data, n * sizeof(float), hipMemcpyHostToDevice, m->stream);
  fwk::launch_f32_to_f16(m->stream, tmp, t->impl.data, (int64_t)n);
  if (he == hipSuccess) he = hipStreamSynchronize(m->stream);
  if (he != hipSuccess) {
    fw_tensor_free(t);
    set_error("tensor_from_host failed: %s", hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  *out = t;
  return FW_OK;
}

void fw_tensor_free(fw_tensor* t) {
  if (!t) return;
  if (t->impl.data) t->impl.pool->give(t->impl.data);   // back to ITS pool, or released when the model is gone
  delete t;
}

// ---------------------------------------------------------------- measurement hooks
void fw_prof_enable(fw_model* fm, int32_t on) {
  if (!fm) return;
  for_each_prof(&fm->impl, [&](Prof& p) { p.on = on != 0; });
}
void fw_prof_reset(fw_model* fm) {
  if (!fm) return;
  for_each_prof(&fm->impl, [](Prof& p) {
    prof_collect(p);
    std::lock_guard<std::mutex> lk(p.mu);
    for (auto& a : p.acc) a = ProfAcc();
  });
}
int32_t fw_prof_count(void) { return PF_COUNT; }
const char* fw_prof_name(int32_t i) { return (i >= 0 && i < PF_COUNT) ? kProfNames[i] : ""; }
int32_t fw_prof_get(fw_model* fm, int32_t i, double* ms, int64_t* launches, double* flops, double* bytes) {
  FW_CHECK_ARG(fm && i >= 0 && i < PF_COUNT, "bad profile index");
  ProfAcc p;
  for_each_prof(&fm->impl, [&](Prof& r) {   // the decode lanes of the group report through their model
    prof_collect(r);
    std::lock_guard<std::mutex> lk(r.mu);
    const ProfAcc& a = r.acc[i];
    p.ms += a.ms; p.launches += a.launches; p.flops += a.flops; p.bytes += a.bytes;
  });
  if (ms) *ms = p.ms;
  if (launches) *launches = p.launches;
  if (flops) *flops = p.flops;
  if (bytes) *bytes = p.bytes;
  return FW_OK;
}
int32_t fw_synchronize(fw_model* fm) {
  FW_CHECK_ARG(fm, "null model");
  FW_HIP(hipSetDevice(fm->impl.device));
  FW_HIP(hipStreamSynchronize(fm->impl.stream));
  for (const auto& l : fm->impl.lanes)
    if (l->stream) FW_HIP(hipStreamSynchronize(l->stream));
  return FW_OK;
}
int32_t fw_dev_alloc(fw_model* fm, int64_t bytes, void** out_dev) {
  FW_CHECK_ARG(fm && out_dev && bytes >= 0, "bad argument");
  FW_HIP(hipSetDevice(fm->impl.device));
  return dev_alloc(out_dev, (size_t)bytes);
}
int32_t fw_dev_free(fw_model* fm, void* dev) {
  FW_CHECK_ARG(fm, "null model");
  FW_HIP(hipSetDevice(fm->impl.device));
  if (dev) FW_HIP(hipFree(dev));
  return FW_OK;
}
int32_t fw_dev_upload(fw_model* fm, void* dst_dev, const void* src_host, int64_t bytes) {
  FW_CHECK_ARG(fm && dst_dev && src_host && bytes >= 0, "bad argument");
  FW_HIP(hipSetDevice(fm->impl.device));
  FW_HIP(hipMemcpy(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice));
  return FW_OK;
}

}  // extern "C"
