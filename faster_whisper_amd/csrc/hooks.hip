// libfwamd.so — the kernel test and bench hooks of include/fwamd_test.h (fw_test_* / fw_bench_*): thin wrappers over
// single kernels on host buffers, through the product's own launchers.  Nothing in the product calls them, and no
// product code lives here (fw_bench_resample is the one hook elsewhere: it is built on resample.hip's private plan).
//
// Every hook owns its device buffers through HookBufs and times launches through time_launches (below): no hook frees,
// creates an event or clears a buffer by hand, so every return path is leak-free.  The model's streams are non-blocking
// streams: a buffer a hook clears before a launch is cleared ON the launch's stream (HookBufs::zero) — a hipMemset on the
// null stream is not ordered against the kernel and may land after its stores.
#include "engine.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "dec_kernels.h"
#include "kernels.h"

using namespace fw;
using fwd::FIN_CAP;
using fwd::GenDev;

namespace {

struct HookBufs : DevBufs {   // device buffers of one hook call, freed on every return path
  template <typename T>
  int upload(T** dst, const T* src, size_t n) {
    int rc = alloc(dst, n);
    if (rc) return rc;
    FW_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return FW_OK;
  }
  int upload_f16(half_t** dst, const float* src, size_t n) {   // rounded to fp16 on the host
    std::vector<half_t> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (half_t)src[i];
    return upload(dst, tmp.data(), n);
  }
  // st: the stream of the launch that follows
  int zero(void* ptr, size_t bytes, hipStream_t st) {
    FW_HIP(hipMemsetAsync(ptr, 0, bytes, st));
    return FW_OK;
  }
};

template <typename T>
int download(T* dst, const T* src, size_t n) {
  FW_HIP(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost));
  return FW_OK;
}
// waits for the launches on st first
int download_f16(hipStream_t st, float* dst, const half_t* src, size_t n) {
  std::vector<half_t> tmp(n);
  FW_HIP(hipStreamSynchronize(st));
  FW_HIP(hipMemcpy(tmp.data(), src, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) dst[i] = (float)tmp[i];
  return FW_OK;
}

// a fragment-major (engine.h: frag_pos) fp16 buffer of ceil(rows / 16) whole tiles, un-permuted into dst [rows][d]
int download_f16_frag(hipStream_t st, float* dst, const half_t* src, int rows, int d) {
  std::vector<float> f((size_t)((rows + 15) / 16 * 16) * d);
  int rc = download_f16(st, f.data(), src, f.size());
  if (rc) return rc;
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < d; ++k) dst[(size_t)r * d + k] = f[frag_pos(r, k, d, 32)];
  return FW_OK;
}

// fragment-major position of key mm, column n (head n / 64) inside one encoder chunk's cross-attention K (vt = false) or
// V^T (vt = true) block of [H][kvp * 64] halves: the layout the projection GEMM's epilogue writes (gemm.hip) and
// dec_cross_attn_kernel / dec_cross_probs_kernel read (dec_kernels.hip, K14).  The one host statement of it: the gemm
// hook un-permutes through it, the cross-attention hooks permute through it.
inline size_t cross_kv_frag_pos(bool vt, int kvp, int mm, int n) {
  const int c = n & 63, r = mm & 31;
  const size_t head = (size_t)(n >> 6) * kvp * 64;
  return vt ? head + ((size_t)((mm >> 5) * 4 + (c >> 4)) * 64 + ((mm >> 3) & 3) * 16 + (c & 15)) * 8 + (mm & 7)
            : head + ((size_t)((mm >> 5) * 4 + 2 * ((r >> 2) & 1) + (c >> 5)) * 64 + ((c >> 3) & 3) * 16 + (((r >> 3) << 2) | (r & 3))) * 8 + (c & 7);
}

// W [N][K] rounded to fp16 and quantised per output row by the weight packer's quantiser (engine.h: quant_row_i8), code
// (n, k) at at(n, k); codes and the [N] de-quantisation scales uploaded
template <typename At>
int upload_quant_w(HookBufs& db, const float* W, int N, int K, At&& at, int8_t** d_wq, float** d_ws) {
  std::vector<int8_t> wq((size_t)N * K);
  std::vector<float> ws(N), row(K);
  for (int n = 0; n < N; ++n) {
    for (int k = 0; k < K; ++k) row[k] = f16_bits_to_f32(f32_to_f16_bits(W[(size_t)n * K + k]));
    ws[n] = quant_row_i8(row.data(), K, wq.data(), [&](int k) { return at(n, k); });
  }
  int rc = db.upload(d_wq, wq.data(), wq.size());
  return rc ? rc : db.upload(d_ws, ws.data(), ws.size());
}

// pseudo-random fp16 fill in [-scale * 1000, scale * 1000) of a device buffer of n halves, staged through `stage`
// (constant fills clock the chip up: MI355X_MICROARCH.md, DVFS)
int fill_lcg(half_t* dst, size_t n, std::vector<uint16_t>& stage, uint32_t seed, float scale) {
  if (stage.size() < n) stage.resize(n);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    stage[i] = f32_to_f16_bits(((int)(seed >> 16) % 2001 - 1000) * scale);
  }
  FW_HIP(hipMemcpy(dst, stage.data(), n * 2, hipMemcpyHostToDevice));
  return FW_OK;
}

// launch(0 .. warmup - 1) untimed, then launch(0 .. iters - 1) between two events on st; *ms_total = the time of the
// `iters` launches together.  A launch(i) that returns non-zero (the launcher refused the shape) ends the run:
// LAUNCH_REFUSED, which no FW_ code equals.  The events are destroyed on every path.
constexpr int LAUNCH_REFUSED = 1;
template <typename F>
int time_launches(hipStream_t st, int warmup, int iters, F&& launch, float* ms_total) {
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  FW_HIP(hipEventCreate(&ev.a));
  FW_HIP(hipEventCreate(&ev.b));
  int lr = 0;
  for (int i = 0; i < warmup && lr == 0; ++i) lr = launch(i);
  FW_HIP(hipEventRecord(ev.a, st));
  for (int i = 0; i < iters && lr == 0; ++i) lr = launch(i);
  FW_HIP(hipEventRecord(ev.b, st));
  FW_HIP(hipEventSynchronize(ev.b));
  if (lr != 0) return LAUNCH_REFUSED;
  FW_HIP(hipEventElapsedTime(ms_total, ev.a, ev.b));
  return FW_OK;
}

int test_layernorm_impl(fw_model* fm, const float* x, const float* g, const float* b, int32_t rows, int32_t d, int32_t frag,
                        float* out) {
  FW_CHECK_ARG(fm && x && g && b && out && rows >= 1, "null argument");
  FW_CHECK_ARG(d % 128 == 0 && d >= 128 && d <= 1536, "d must be a multiple of 128 and <= 1536");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  half_t *dx, *dg, *dlb, *dy;
  const size_t ny = (size_t)(frag ? (rows + 15) / 16 * 16 : rows) * d;   // the fragment-major form is whole 16-row tiles
  int rc;
  if ((rc = db.upload_f16(&dx, x, (size_t)rows * d)) || (rc = db.upload_f16(&dg, g, d)) || (rc = db.upload_f16(&dlb, b, d)) ||
      (rc = db.alloc(&dy, ny)) || (rc = db.zero(dy, ny * sizeof(half_t), m->stream)))
    return rc;
  fwk::launch_layernorm(m->stream, dx, dg, dlb, dy, rows, d, frag ? 1 : 0);
  return frag ? download_f16_frag(m->stream, out, dy, rows, d) : download_f16(m->stream, out, dy, (size_t)rows * d);
}

}  // namespace

extern "C" {

int32_t fw_test_gemm(fw_model* fm, const float* A, const float* W, const float* bias, const float* residual,
                     int32_t M, int32_t N, int32_t K, int32_t act_gelu, int32_t use_int8, float* out) {
  FW_CHECK_ARG(fm && A && W && out, "null argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const bool frag_kv = !use_int8 && (act_gelu == 8 || act_gelu == 9);
  FW_CHECK_ARG(!use_int8 || m->compute_type == FW_COMPUTE_INT8_FLOAT16, "int8 gemm test needs an int8_float16 model");
  if (frag_kv && (N % 64 || residual)) { set_error("fragment-major gemm test: N %% 64 == 0, no residual"); return FW_EINVAL; }
  HookBufs db;
  half_t *dA, *dW, *dB = nullptr, *dR = nullptr, *dC;
  int rc;
  if ((rc = db.upload_f16(&dA, A, (size_t)M * K)) || (rc = db.upload_f16(&dW, W, (size_t)N * K)) ||
      (bias && (rc = db.upload_f16(&dB, bias, N))) || (residual && (rc = db.upload_f16(&dR, residual, (size_t)M * N))) ||
      (rc = db.alloc(&dC, (size_t)M * N)))
    return rc;
  LinearW L{dW, dB, nullptr, nullptr, nullptr, nullptr, N, K};
  LinIn in{dA, K, 0};
  if (use_int8) {
    int8_t* dWq;
    float* dWs;
    if ((rc = upload_quant_w(db, W, N, K, [&](int n, int k) { return (size_t)n * K + k; }, &dWq, &dWs)) ||
        (rc = quantise_rows(m, dA, nullptr, M, K, nullptr, m->ws_xq)))
      return rc;
    L.wq = dWq; L.wscale = dWs;
    in = {.xq = &m->ws_xq};
  }
  if (frag_kv) {
    // the cross-attention K (8) / V^T (9) projection epilogues: output MFMA-fragment-major per 64-column head
    // (gemm.hip), un-permuted here into out [M][N]; the padded keys of the last 32-key group must stay zero
    const bool vt = act_gelu == 9;
    const int kvp = (M + 31) / 32 * 32, H = N / 64;
    std::vector<float> hf((size_t)H * kvp * 64);
    half_t* dF;
    if ((rc = db.alloc(&dF, hf.size())) || (rc = db.zero(dF, hf.size() * sizeof(half_t), m->stream))) return rc;
    if ((rc = run_linear(m, L, {.in = in, .C = dF, .ldc = vt ? kvp : N, .M = M, .trans = vt, .head_rows = kvp})) ||
        (rc = download_f16(m->stream, hf.data(), dF, hf.size())))
      return rc;
    for (int mm = 0; mm < kvp; ++mm)
      for (int n = 0; n < N; ++n) {
        const size_t off = cross_kv_frag_pos(vt, kvp, mm, n);
        if (mm < M) out[(size_t)mm * N + n] = hf[off];
        else if (hf[off] != 0.f) { set_error("fragment-major epilogue wrote the padded key %d", mm); return FW_ERUNTIME; }
      }
    return FW_OK;
  }
  const bool trans = act_gelu >= 2;   // transposed-output mode: out is [N][M], act = act_gelu - 2, no residual
  rc = run_linear(m, L, {.in = in, .C = dC, .ldc = trans ? M : N, .res = trans ? nullptr : dR, .ldr = trans ? 0 : N, .M = M,
                         .act = trans ? act_gelu - 2 : act_gelu, .trans = trans});
  return rc ? rc : download_f16(m->stream, out, dC, (size_t)M * N);
}

int32_t fw_test_dec_linear(fw_model* fm, const float* x, const float* W, const float* bias, const float* ln_g,
                           const float* ln_b, const float* res, int32_t R, int32_t N, int32_t K, int32_t act,
                           int32_t form, float* out, float* out_from_frag) {
  FW_CHECK_ARG(fm && x && W && out && out_from_frag, "null argument");
  FW_CHECK_ARG(R >= 1 && N % 32 == 0 && K % 64 == 0, "need R >= 1, N %% 32 == 0, K %% 64 == 0");
  FW_CHECK_ARG((ln_g == nullptr) == (ln_b == nullptr), "ln_g and ln_b go together");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const bool i8 = form == 1;   // (1 is no DecLinForm: the int8 kernel on an int8_float16 model)
  if (i8 && (m->compute_type != FW_COMPUTE_INT8_FLOAT16 || ln_g)) {
    set_error("int8 decoder-linear test needs an int8_float16 model and no LayerNorm");
    return FW_EINVAL;
  }
  hipStream_t st = m->stream;
  const int R16 = (R + 15) / 16 * 16;
  auto h = [](float v) { return f16_bits_to_f32(f32_to_f16_bits(v)); };
  HookBufs db;
  half_t *d_res = nullptr, *d_bias = nullptr, *d_out;
  int rc;
  if ((res && (rc = db.upload_f16(&d_res, res, (size_t)R * N))) || (rc = db.alloc(&d_out, (size_t)R * N))) return rc;
  if (i8) {
    int8_t *d_wq, *d_xq;
    float *d_ws, *d_xs;
    half_t* d_x;
    if ((rc = upload_quant_w(db, W, N, K, [&](int n, int k) { return frag_pos(n, k, K, 64); }, &d_wq, &d_ws)) ||
        (rc = db.upload_f16(&d_x, x, (size_t)R * K)) || (bias && (rc = db.upload_f16(&d_bias, bias, N))) ||
        (rc = db.alloc(&d_xq, (size_t)R16 * K)) || (rc = db.alloc(&d_xs, (size_t)R16)) || (rc = db.zero(d_xq, (size_t)R16 * K, st)))
      return rc;
    fwk::launch_quant_rows(st, d_x, K, nullptr, nullptr, d_xq, d_xs, R, K, 1);
    if (fwd::launch_dec_gemm_frag_i8(st, d_xq, d_xs, d_wq, d_ws, d_bias, d_res, N, d_out, N, R, N, K, act) != 0) {
      set_error("int8 decoder linear: unsupported shape R=%d N=%d K=%d", R, N, K);
      return FW_ERUNTIME;
    }
    if ((rc = download_f16(st, out, d_out, (size_t)R * N))) return rc;
    memcpy(out_from_frag, out, (size_t)R * N * sizeof(float));
    return FW_OK;
  }
  // fp16: fold the LayerNorm exactly like the weight packer (engine.hip: Packer::folded)
  std::vector<uint16_t> wf((size_t)N * K), xf((size_t)R16 * K, 0);
  std::vector<float> s1(N, 0.f), cf(N, 0.f);
  for (int n = 0; n < N; ++n) {
    double a1 = 0.0, ac = 0.0;
    for (int k = 0; k < K; ++k) {
      const float wv = h(W[(size_t)n * K + k]);
      const uint16_t wg = ln_g ? f32_to_f16_bits(wv * h(ln_g[k])) : f32_to_f16_bits(wv);
      wf[frag_pos(n, k, K, 32)] = wg;
      a1 += (double)f16_bits_to_f32(wg);
      if (ln_g) ac += (double)wv * (double)h(ln_b[k]);
    }
    if (bias) ac += (double)h(bias[n]);
    s1[n] = (float)a1;
    cf[n] = (float)ac;
  }
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < K; ++k) xf[frag_pos(r, k, K, 32)] = f32_to_f16_bits(x[(size_t)r * K + k]);
  uint16_t *d_wf, *d_xf;
  half_t* d_of;
  float *d_s1 = nullptr, *d_cf = nullptr;
  if ((rc = db.upload(&d_wf, wf.data(), wf.size())) || (rc = db.upload(&d_xf, xf.data(), xf.size())) ||
      (rc = db.alloc(&d_of, (size_t)R16 * N)) || (rc = db.zero(d_of, (size_t)R16 * N * 2, st)))
    return rc;
  if (ln_g) {
    if ((rc = db.upload(&d_s1, s1.data(), (size_t)N)) || (rc = db.upload(&d_cf, cf.data(), (size_t)N))) return rc;
  } else if (bias) {
    if ((rc = db.upload_f16(&d_bias, bias, N))) return rc;
  }
  // form: fwd::DecLinForm (0: the product's choice; 5: the skinny kernel whatever the row count, the reference of the
  // bit-identity test; 6 / 7: its tile groupings; 10 + cfg: the GEMM-shaped kernel of merged runs)
  const fwd::DecLin lin{(const half_t*)d_xf, (const half_t*)d_wf, d_bias, d_s1, d_cf, d_res, N, d_out, N, d_of, R, N, K, act};
  if (fwd::launch_dec_linear(st, lin, form) != 0) {
    set_error("decoder linear: unsupported shape R=%d N=%d K=%d (form %d)", R, N, K, form);
    return FW_ERUNTIME;
  }
  if ((rc = download_f16(st, out, d_out, (size_t)R * N))) return rc;
  return download_f16_frag(st, out_from_frag, d_of, R, N);
}

int32_t fw_dec_big_min_rows(void) { return fwd::dec_big_min_rows(); }
int32_t fw_dec_big_min_rows_of(int32_t role, int32_t compute_type) { return fwd::dec_big_min_rows_of(role, compute_type); }

// process-wide measurement knobs (A/B inside one process: profiles/gemm_bench.py); 1: encoder GEMM tile order
int32_t fw_test_knob(int32_t id, int32_t value) {
  FW_CHECK_ARG(id == 1 || id == 2 || id == 4 || id == 5 || id == 6 || id == 7, "unknown knob %d", id);
  if (id == 6) { set_cross_kv_layered(value); return FW_OK; }
  if (id == 7) { fwd::set_cross_attn_regs(value); return FW_OK; }
  if (id == 1) fwk::g_gemm_order.store(value);
  else if (id == 5) fwk::g_gemm_vt_stage.store(value);
  else if (id == 2) fwd::set_self_attn_form(value);
  else set_pos_blocks(value);
  return FW_OK;
}

// host-only: the run size an idle two-lane decode group leads with (decoder.hip: idle_lead_chunks); needs no device
int64_t fw_test_idle_lead_chunks(int64_t queued, int32_t n_queued, int32_t encoding, int64_t want, int32_t max_batch) {
  return idle_lead_chunks(queued, n_queued, encoding, want, max_batch);
}

// host-only: what a lane holds of runs led by one call (decoder.hip: RunCapacity); needs no device
int32_t fw_test_run_capacity(int32_t lane_chunks, int32_t max_batch, int32_t max_beam, int64_t self_cap, int32_t B,
                             int32_t sampling, int32_t beam_size, int32_t num_hypotheses, int32_t ctx,
                             int64_t* rows_per_chunk, int64_t* want, int64_t* run_cap) {
  const RunCapacity cap(lane_chunks, max_batch, max_beam, self_cap, B, sampling != 0, beam_size, num_hypotheses, ctx);
  *rows_per_chunk = cap.rows_per_chunk;
  *want = cap.want;
  *run_cap = cap.run_cap;
  return cap.rows_fit && cap.cache_fits ? 1 : 0;
}

// host-only: the form a decoder linear takes (dec_kernels.hip: dec_linear_plan); needs no device
int32_t fw_test_dec_linear_plan(int32_t R, int32_t N, int32_t K, int32_t ldo, int32_t ldr, int32_t compute_type,
                                int32_t form, int32_t out[6]) {
  const fwd::DecLinPlan p = fwd::dec_linear_plan(R, N, K, ldo, ldr, compute_type, form);
  const int32_t f[6] = {p.family, p.cfg, p.row_tiles, p.col_tiles, p.chunk, p.waves};
  memcpy(out, f, sizeof(f));
  return FW_OK;
}

// host-only: what a launch of the encoder GEMM does (gemm.hip: gemm_plan); needs no device
int32_t fw_test_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t batch, int64_t lda, int64_t ldw, int64_t a_bstride,
                          int64_t ldc, int64_t c_bstride, int32_t trans, int32_t int8, int32_t head_rows, int32_t n_layers,
                          int32_t has_res, int32_t out[9]) {
  static const float some_scale = 1.f;   // (the plan asks only whether the pointers are set)
  static const half_t some_res = 0;
  fwk::GemmParams p{};
  p.lda = lda; p.a_bstride = a_bstride; p.ldw = ldw; p.ldc = ldc; p.c_bstride = c_bstride;
  p.M = M; p.N = N; p.K = K;
  p.head_rows = head_rows; p.n_layers = n_layers;
  p.a_scale = int8 ? &some_scale : nullptr;
  p.w_scale = int8 == 1 ? &some_scale : nullptr;
  p.res = has_res ? &some_res : nullptr;
  const fwk::GemmPlan pl = fwk::gemm_plan(p, batch, trans != 0);
  const int32_t f[9] = {pl.kernel, pl.p.nMt, pl.p.nNt, pl.p.nNt_layer, pl.p.n_mp, pl.p.blk_n, pl.p.blk_m, pl.p.vt_stage, pl.grid};
  memcpy(out, f, sizeof(f));   // (a refused shape: kernel -1, the rest as passed in: 0)
  return FW_OK;
}

// host-only: the form a decode step's self-attention takes (dec_kernels.hip: self_attn_form); needs no device
int32_t fw_test_self_attn_form(int32_t n_ctx, int32_t cache_ctx, int32_t d, int32_t R_total, int32_t kmul, int32_t H,
                               int32_t chunks, int32_t knob) {
  return fwd::self_attn_form(n_ctx, cache_ctx, d, R_total, kmul, H, chunks, knob);
}

// host-only: what model creation checks of a blob before it binds it (engine.hip), on a host copy; needs no device
int32_t fw_test_blob_check(const void* blob_host, int64_t bytes) {
  FW_CHECK_ARG(blob_host && bytes >= (int64_t)sizeof(BlobHeader), "weight blob too small");
  BlobHeader h;
  memcpy(&h, blob_host, sizeof(h));
  if (int rc = check_blob_header(h, bytes)) return rc;
  std::vector<BlobEntry> entries(h.n_tensors);
  memcpy(entries.data(), reinterpret_cast<const char*>(blob_host) + sizeof(h), entries.size() * sizeof(BlobEntry));
  Weights unused;
  bool has_plain;
  return bind_weights(h, entries.data(), const_cast<void*>(blob_host), unused, &has_plain);
}

int32_t fw_test_dec_logits(fw_model* fm, const float* x, int32_t R, float* out) {
  FW_CHECK_ARG(fm && x && out && R >= 1, "bad argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int d = m->cfg.d_model, V = m->cfg.n_vocab, R16 = (R + 15) / 16 * 16;
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  std::vector<half_t> xh((size_t)R16 * d, (half_t)0.f);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < d; ++k) xh[i8 ? (size_t)r * d + k : frag_pos(r, k, d, 32)] = (half_t)x[(size_t)r * d + k];
  HookBufs db;
  half_t* d_x;
  float* d_out;
  int rc, lr;
  if ((rc = db.upload(&d_x, xh.data(), xh.size())) || (rc = db.alloc(&d_out, (size_t)R * V))) return rc;
  if (i8) {
    int8_t* d_xq;
    float* d_xs;
    if ((rc = db.alloc(&d_xq, (size_t)R16 * d)) || (rc = db.alloc(&d_xs, (size_t)R16)) || (rc = db.zero(d_xq, (size_t)R16 * d, st)))
      return rc;
    fwk::launch_quant_rows(st, d_x, d, m->dec_ln.g, m->dec_ln.b, d_xq, d_xs, R, d, 1);
    lr = fwd::launch_dec_logits(st, true, d_xq, d_xs, m->logits.wq, m->logits.wscale, nullptr, nullptr, d_out, V, R, V, d);
  } else {
    lr = fwd::launch_dec_logits(st, false, d_x, nullptr, m->logits.w, nullptr, m->logits.s1, m->logits.cf, d_out, V, R, V,
                                d);
  }
  FW_HIP(hipStreamSynchronize(st));
  if (lr != 0) {
    set_error("logits projection test failed: unsupported shape");
    return FW_ERUNTIME;
  }
  return download(out, d_out, (size_t)R * V);
}

// Micro-benchmark of the decoder linear kernel's tile shapes (profiles/dec_linear_bench.py): `iters` back-to-back
// launches on one stream over a ROTATING set of weight matrices larger than L2 + MALL (as in a decode step, where
// 1.5 GB of weights pass between two uses of the same matrix); us_out = mean microseconds per launch.
int32_t fw_bench_dec_linear(fw_model* fm, int32_t R, int32_t N, int32_t K, int32_t lnf, int32_t variant, int32_t iters,
                            float* us_out) {
  FW_CHECK_ARG(fm && us_out && R > 0 && N > 0 && K > 0 && iters > 0, "bad argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t wn = (size_t)N * K;
  const int copies = (int)std::max<size_t>(2, ((size_t)640 << 20) / (wn * 2));
  const size_t rp = ((size_t)R + 15) / 16 * 16;
  HookBufs db;
  half_t *dW, *dX, *dO, *dB;
  float *dS, *dC;
  std::vector<uint16_t> stage;
  int rc;
  if ((rc = db.alloc(&dW, wn * copies)) || (rc = db.alloc(&dX, rp * K)) || (rc = db.alloc(&dO, rp * N)) ||
      (rc = db.alloc(&dB, (size_t)N)) || (rc = db.alloc(&dS, (size_t)N)) || (rc = db.alloc(&dC, (size_t)N)) ||
      (rc = fill_lcg(dW, wn, stage, 2463534242u, 1e-3f)) || (rc = fill_lcg(dX, rp * K, stage, 2463534242u, 1e-3f)) ||
      (rc = db.zero(dB, (size_t)N * 2, st)) || (rc = db.zero(dS, (size_t)N * 4, st)) || (rc = db.zero(dC, (size_t)N * 4, st)))
    return rc;
  for (int c = 1; c < copies; ++c) FW_HIP(hipMemcpy(dW + (size_t)c * wn, dW, wn * 2, hipMemcpyDeviceToDevice));
  float ms = 0.f;
  rc = time_launches(st, 4, iters, [&](int i) {
    return fwd::launch_dec_gemm_frag_variant(st, variant, lnf != 0, dX, dW + (size_t)(i % copies) * wn, dB, dS, dC, dO, R, N, K);
  }, &ms);
  if (rc == LAUNCH_REFUSED) { set_error("fw_bench_dec_linear: unsupported shape / variant"); return FW_EINVAL; }
  if (rc) return rc;
  *us_out = ms * 1000.f / (float)iters;
  return FW_OK;
}

// measurement hook (profiles/gemm_bench.py): the encoder GEMM on device-resident pseudo-random operands,
// `iters` launches between two events.  lda = K + a_pad, ldw = K + w_pad elements (stride experiments).
int32_t fw_bench_gemm(fw_model* fm, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t a_pad, int32_t w_pad,
                      int32_t trans, int32_t iters, float* ms_out) {
  FW_CHECK_ARG(fm && ms_out && M > 0 && N > 0 && K > 0 && batch > 0 && iters > 0, "bad argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  const int64_t lda = K + a_pad, ldw = K + w_pad;
  // transposed output: Ct[z][n][m] with the row stride the encoder's V^T has (keys padded to a multiple of 64: t_pad)
  const int64_t ldct = (M + 63) / 64 * 64;
  const size_t na = (size_t)batch * M * lda, nw = (size_t)N * ldw,
               nc = trans ? (size_t)batch * N * ldct : (size_t)batch * M * N;
  // A and W in halves: an int8 model reads the same bytes as codes, two to a half
  const size_t ha = i8 ? (na + 1) / 2 : na, hw = i8 ? (nw + 1) / 2 : nw;
  HookBufs db;
  half_t *dA, *dW, *dC;
  float *dsa = nullptr, *dsw = nullptr;
  std::vector<uint16_t> stage;
  int rc;
  if ((rc = db.alloc(&dA, ha)) || (rc = db.alloc(&dW, hw)) || (rc = db.alloc(&dC, nc)) ||
      (rc = fill_lcg(dA, ha, stage, 12345u, 1e-3f)) || (rc = fill_lcg(dW, hw, stage, 12345u, 1e-3f)))
    return rc;
  if (i8 && ((rc = db.alloc(&dsa, (size_t)batch * M)) || (rc = db.alloc(&dsw, (size_t)N)) ||
             (rc = db.zero(dsa, (size_t)batch * M * 4, m->stream)) || (rc = db.zero(dsw, (size_t)N * 4, m->stream))))
    return rc;
  // (int8: the same bytes as codes, behind a record that describes them — rows of ld = lda codes — without owning them)
  QuantRows xq;
  xq.q = reinterpret_cast<int8_t*>(dA); xq.scale = dsa; xq.ld = lda;
  const LinearW L{dW, nullptr, reinterpret_cast<const int8_t*>(dW), dsw, nullptr, nullptr, N, K};
  LinCall call{.C = dC, .ldc = trans ? ldct : N, .c_bs = trans ? (int64_t)N * ldct : (int64_t)M * N, .M = M};
  if (i8) call.in = {.xq = &xq};
  else call.in = {dA, lda, (int64_t)M * lda};
  const fwk::GemmParams p = gemm_params(L, call, ldw);
  float ms = 0.f;
  rc = time_launches(m->stream, 1, iters, [&](int) { return fwk::launch_gemm(m->stream, p, batch, trans != 0); }, &ms);
  if (rc == LAUNCH_REFUSED) { set_error("gemm bench failed: unsupported shape"); return FW_ERUNTIME; }
  if (rc) return rc;
  *ms_out = ms / (float)iters;
  return FW_OK;
}

// measurement hook (profiles/gemm_bench.py --epilogue): fw_bench_gemm with the epilogue the PRODUCT runs for the shape —
// bias, GELU, residual as run_encoder passes them, or (n_layers > 1) the layered head-major cross-attention K / V^T
// projection of ensure_cross_kv.  The residual is read from a set of buffers larger than L2 + MALL, rotated launch by
// launch (res = 1), or from one [M][N] block shared by the chunks (res = 2: conv2's positional embedding).
int32_t fw_bench_gemm_epi(fw_model* fm, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t lda_in, int32_t trans,
                          int32_t bias, int32_t act, int32_t res, int32_t n_layers, int32_t iters, float* ms_out) {
  FW_CHECK_ARG(fm && ms_out && M > 0 && N > 0 && K > 0 && batch > 0 && iters > 0 && n_layers >= 1, "bad argument");
  FW_CHECK_ARG(res >= 0 && res <= 2 && !(res && (trans || n_layers > 1)), "residual: row-major single-layer output only");
  Model* m = &fm->impl;
  FW_CHECK_ARG(m->compute_type != FW_COMPUTE_INT8_FLOAT16, "float16 models only");
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const int64_t lda = lda_in > 0 ? lda_in : K;
  const bool layered = n_layers > 1;
  const int64_t kvp = (M + 31) / 32 * 32;                  // keys of a head, padded to whole 32-key groups (the pool's kvp)
  const int64_t ldct = layered ? kvp : (M + 63) / 64 * 64;
  const int64_t c_bs = layered ? (int64_t)N * kvp : (trans ? (int64_t)N * ldct : (int64_t)M * N);
  const int64_t c_ls = c_bs * batch;
  const size_t na = (size_t)batch * ((size_t)M * lda + K), nw = (size_t)N * K * n_layers, nc = (size_t)c_ls * n_layers;
  const size_t nr1 = res == 1 ? (size_t)batch * M * N : (size_t)M * N;
  const int copies = res == 1 ? (int)std::max<size_t>(2, ((size_t)640 << 20) / (nr1 * 2)) : 1;
  HookBufs db;
  half_t *dA, *dW, *dC, *dB, *dR = nullptr;
  std::vector<uint16_t> stage;
  int rc;
  if ((rc = db.alloc(&dA, na)) || (rc = db.alloc(&dW, nw)) || (rc = db.alloc(&dC, nc)) || (rc = db.alloc(&dB, (size_t)N * n_layers)) ||
      (res && (rc = db.alloc(&dR, nr1 * copies))) || (rc = fill_lcg(dA, na, stage, 12345u, 1e-3f)) ||
      (rc = fill_lcg(dW, nw, stage, 12345u, 1e-3f)) || (rc = fill_lcg(dB, (size_t)N * n_layers, stage, 777u, 1e-3f)) ||
      (res && (rc = fill_lcg(dR, nr1, stage, 4242u, 1e-3f))) || (rc = db.zero(dC, nc * 2, m->stream)))
    return rc;
  for (int c = 1; res && c < copies; ++c) FW_HIP(hipMemcpy(dR + (size_t)c * nr1, dR, nr1 * 2, hipMemcpyDeviceToDevice));
  const LinearW L{dW, bias ? dB : nullptr, nullptr, nullptr, nullptr, nullptr, N, K};
  LinCall call{.in = {dA, lda, (int64_t)M * lda}, .C = dC, .ldc = trans ? ldct : N, .c_bs = c_bs, .ldr = N,
               .r_bs = res == 1 ? (int64_t)M * N : 0, .M = M, .act = act};
  if (layered) {
    call.head_rows = (int)kvp;
    call.n_layers = n_layers; call.w_ls = (int64_t)N * K; call.b_ls = N; call.c_ls = c_ls;
  }
  float ms = 0.f;
  rc = time_launches(m->stream, 1, iters, [&](int i) {
    call.res = res ? dR + (size_t)(i % copies) * nr1 : nullptr;
    return fwk::launch_gemm(m->stream, gemm_params(L, call, K), batch, trans != 0);
  }, &ms);
  if (rc == LAUNCH_REFUSED) { set_error("gemm epilogue bench failed: unsupported shape"); return FW_ERUNTIME; }
  if (rc) return rc;
  *ms_out = ms / (float)iters;
  return FW_OK;
}

// measurement hook (profiles/dec_linear_bench.py --epilogue): fw_bench_dec_linear with the epilogue a decode step runs —
// act, and with res = 1 the residual added IN PLACE (res == out, as run_step passes g->x), outs bit 0 / 1: the row-major
// / the fragment-major copy written.  Weights AND the in-place residual / output rows rotate over sets larger than
// L2 + MALL.  variant 0: what a decode step launches for this row count; 5: the register-streaming kernel; 10 + cfg:
// the GEMM-shaped kernel of merged runs.
int32_t fw_bench_dec_linear_epi(fw_model* fm, int32_t R, int32_t N, int32_t K, int32_t lnf, int32_t variant, int32_t act,
                                int32_t res, int32_t outs, int32_t iters, float* us_out) {
  FW_CHECK_ARG(fm && us_out && R > 0 && N > 0 && K > 0 && iters > 0, "bad argument");
  FW_CHECK_ARG((outs & 3) != 0 && (!res || (outs & 1)), "needs an output; the residual is the row-major output in place");
  FW_CHECK_ARG(variant == 0 || variant == 5 || (variant >= 10 && variant <= 12), "unknown variant %d", variant);
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t wn = (size_t)N * K;
  const int copies = (int)std::max<size_t>(2, ((size_t)640 << 20) / (wn * 2));
  const size_t rp = ((size_t)R + 15) / 16 * 16, on = rp * N;
  const int ocopies = (int)std::max<size_t>(2, ((size_t)640 << 20) / (on * 2));
  HookBufs db;
  half_t *dW, *dX, *dO, *dF, *dB;
  float *dS, *dC;
  std::vector<uint16_t> stage;
  int rc;
  // (zero residual / bias / fold constants: an in-place residual that is re-read iters / ocopies times stays finite)
  if ((rc = db.alloc(&dW, wn * copies)) || (rc = db.alloc(&dX, rp * K)) || (rc = db.alloc(&dO, on * ocopies)) ||
      (rc = db.alloc(&dF, on)) || (rc = db.alloc(&dB, (size_t)N)) || (rc = db.alloc(&dS, (size_t)N)) || (rc = db.alloc(&dC, (size_t)N)) ||
      (rc = fill_lcg(dW, wn, stage, 2463534242u, 1e-3f)) || (rc = fill_lcg(dX, rp * K, stage, 2463534242u, 1e-3f)) ||
      (rc = db.zero(dO, on * ocopies * 2, st)) || (rc = db.zero(dB, (size_t)N * 2, st)) || (rc = db.zero(dS, (size_t)N * 4, st)) ||
      (rc = db.zero(dC, (size_t)N * 4, st)))
    return rc;
  for (int c = 1; c < copies; ++c) FW_HIP(hipMemcpy(dW + (size_t)c * wn, dW, wn * 2, hipMemcpyDeviceToDevice));
  float ms = 0.f;
  rc = time_launches(st, 4, iters, [&](int i) {
    const half_t* w = dW + (size_t)(i % copies) * wn;
    half_t* o = dO + (size_t)(i % ocopies) * on;
    half_t* op = (outs & 1) ? o : nullptr;
    half_t* of = (outs & 2) ? dF : nullptr;
    const half_t* r = res ? o : nullptr;
    const half_t* b = lnf ? nullptr : dB;
    const float *s1 = lnf ? dS : nullptr, *cf = lnf ? dC : nullptr;
    return fwd::launch_dec_linear(st, fwd::DecLin{dX, w, b, s1, cf, r, N, op, N, of, R, N, K, act}, variant);
  }, &ms);
  if (rc == LAUNCH_REFUSED) { set_error("fw_bench_dec_linear_epi: unsupported shape / variant"); return FW_EINVAL; }
  if (rc) return rc;
  *us_out = ms * 1000.f / (float)iters;
  return FW_OK;
}

int32_t fw_test_layernorm(fw_model* fm, const float* x, const float* g, const float* b, int32_t rows, int32_t d,
                          float* out) {
  return test_layernorm_impl(fm, x, g, b, rows, d, 0, out);
}
int32_t fw_test_layernorm_frag(fw_model* fm, const float* x, const float* g, const float* b, int32_t rows, int32_t d,
                               int32_t frag, float* out) {
  return test_layernorm_impl(fm, x, g, b, rows, d, frag, out);
}

int32_t fw_test_quant_rows(fw_model* fm, const float* x, int32_t rows, int32_t d, int64_t ldx, const float* ln_g,
                           const float* ln_b, int32_t frag, int8_t* xq, float* scale) {
  FW_CHECK_ARG(fm && x && xq && scale && rows >= 1 && rows <= (1 << 20), "bad argument");
  FW_CHECK_ARG((ln_g == nullptr) == (ln_b == nullptr), "ln_g and ln_b go together");
  FW_CHECK_ARG(d >= 64 && d % 64 == 0 && d <= (ln_g ? 1536 : 5120), "d %% 64 == 0, d <= 1536 with LayerNorm, <= 5120 without");
  FW_CHECK_ARG(ldx >= d && ldx % 8 == 0 && ldx <= (1 << 20), "ldx >= d, ldx %% 8 == 0");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const int R16 = (rows + 15) / 16 * 16;
  std::vector<int8_t> hq((size_t)R16 * d);
  HookBufs db;
  half_t *dx, *dg = nullptr, *dlb = nullptr;
  int8_t* dq;
  float* ds;
  int rc;
  if ((rc = db.upload_f16(&dx, x, (size_t)(rows - 1) * ldx + d)) || (ln_g && (rc = db.upload_f16(&dg, ln_g, d))) ||
      (ln_b && (rc = db.upload_f16(&dlb, ln_b, d))) || (rc = db.alloc(&dq, hq.size())) || (rc = db.alloc(&ds, (size_t)R16)) ||
      (rc = db.zero(dq, hq.size(), m->stream)))
    return rc;
  fwk::launch_quant_rows(m->stream, dx, ldx, dg, dlb, dq, ds, rows, d, frag ? 1 : 0);
  FW_HIP(hipStreamSynchronize(m->stream));
  if ((rc = download(hq.data(), dq, hq.size())) || (rc = download(scale, ds, (size_t)rows))) return rc;
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < d; ++k) xq[(size_t)r * d + k] = hq[frag ? frag_pos(r, k, d, 64) : (size_t)r * d + k];
  return FW_OK;
}

int32_t fw_test_cross_kv_frag_index(int32_t vt, int32_t kvp, int32_t N, int64_t* idx) {
  FW_CHECK_ARG(idx && kvp >= 32 && kvp % 32 == 0 && N >= 64 && N % 64 == 0, "need kvp %% 32 == 0, N %% 64 == 0");
  for (int mm = 0; mm < kvp; ++mm)
    for (int n = 0; n < N; ++n) idx[(size_t)mm * N + n] = (int64_t)cross_kv_frag_pos(vt != 0, kvp, mm, n);
  return FW_OK;
}

int32_t fw_test_gemm_ex(fw_model* fm, const float* A, int64_t a_elems, int64_t lda, int64_t a_bstride, const float* W,
                        const float* bias, const float* res, int64_t r_elems, int64_t ldr, int64_t r_bstride, float* C,
                        int64_t c_elems, int64_t c_off, int64_t ldc, int64_t c_bstride, int64_t c_lstride, int32_t M,
                        int32_t N, int32_t K, int32_t batch, int32_t n_layers, int32_t act, int32_t trans,
                        int32_t head_rows, int32_t use_int8, const float* ln_g, const float* ln_b) {
  FW_CHECK_ARG(fm && A && W && C, "null argument");
  const int64_t dim_max = 1 << 20, cnt_max = 1 << 12, str_max = (int64_t)1 << 40;   // (no product below can overflow)
  FW_CHECK_ARG(M >= 1 && N >= 1 && K >= 1 && M <= dim_max && N <= dim_max && K <= dim_max, "bad M / N / K");
  FW_CHECK_ARG(batch >= 1 && n_layers >= 1 && batch <= cnt_max && n_layers <= cnt_max, "bad batch / n_layers");
  for (int64_t v : {a_elems, lda, a_bstride, r_elems, ldr, r_bstride, c_elems, c_off, ldc, c_bstride, c_lstride})
    FW_CHECK_ARG(v >= 0 && v <= str_max, "negative or oversized count / stride");
  FW_CHECK_ARG(act == 0 || act == 1, "act is 0 or 1");
  FW_CHECK_ARG((ln_g == nullptr) == (ln_b == nullptr) && (!ln_g || use_int8), "ln_g / ln_b: both, and only with use_int8");
  const bool rowmajor = !trans && head_rows == 0;
  FW_CHECK_ARG(!res || (rowmajor && n_layers == 1), "a residual needs the row-major single-layer form");
  FW_CHECK_ARG(n_layers == 1 || (!use_int8 && act == 0), "the layered launch is fp16 without activation");
  FW_CHECK_ARG(head_rows == 0 || (head_rows > 0 && head_rows % 32 == 0 && head_rows >= M && N % 64 == 0),
               "fragment-major output: head_rows %% 32 == 0, head_rows >= M, N %% 64 == 0");
  // 16-byte stores of the epilogues start from these offsets
  FW_CHECK_ARG(c_off % 8 == 0 && c_lstride % 8 == 0, "c_off and c_lstride must be multiples of 8");
  if (use_int8) FW_CHECK_ARG(lda == K && a_bstride == (int64_t)M * K, "int8: A is contiguous [batch * M][K]");
  // ---- the furthest element the launch touches in each buffer (gemm.hip: rows are clamped to M - 1, every K tile is read
  // whole, residual and output are touched only at m < M, n < N; a fragment-major key group is written as a whole) ----
  const int64_t a_last = (int64_t)(batch - 1) * a_bstride + (int64_t)(M - 1) * lda + (K - 1);
  FW_CHECK_ARG(a_last < a_elems, "the launch reads A[%lld], a_elems = %lld", (long long)a_last, (long long)a_elems);
  if (res) {
    const int64_t r_last = (int64_t)(batch - 1) * r_bstride + (int64_t)(M - 1) * ldr + (N - 1);
    FW_CHECK_ARG(r_last < r_elems, "the launch reads res[%lld], r_elems = %lld", (long long)r_last, (long long)r_elems);
  }
  const int64_t chunk_last = head_rows > 0 ? (int64_t)(N / 64 - 1) * head_rows * 64 + (int64_t)((M - 1) / 32 + 1) * 2048 - 1
                             : trans       ? (int64_t)(N - 1) * ldc + (M - 1)
                                           : (int64_t)(M - 1) * ldc + (N - 1);
  const int64_t c_last = c_off + (int64_t)(n_layers - 1) * c_lstride + (int64_t)(batch - 1) * c_bstride + chunk_last;
  FW_CHECK_ARG(c_last < c_elems, "the launch writes C[%lld], c_elems = %lld", (long long)c_last, (long long)c_elems);

  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_CHECK_ARG(!use_int8 || (m->compute_type == FW_COMPUTE_INT8_FLOAT16 && !(ln_g && K > 1536)),
               "int8 gemm test needs an int8_float16 model, K <= 1536 with LayerNorm");
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  half_t *dA, *dW, *dB = nullptr, *dR = nullptr, *dC, *dG = nullptr, *dLb = nullptr;
  int rc;
  if ((rc = db.upload_f16(&dA, A, (size_t)a_elems)) || (rc = db.upload_f16(&dW, W, (size_t)n_layers * N * K)) ||
      (bias && (rc = db.upload_f16(&dB, bias, (size_t)n_layers * N))) || (res && (rc = db.upload_f16(&dR, res, (size_t)r_elems))) ||
      (rc = db.upload_f16(&dC, C, (size_t)c_elems)) ||
      (ln_g && ((rc = db.upload_f16(&dG, ln_g, K)) || (rc = db.upload_f16(&dLb, ln_b, K)))))
    return rc;
  LinearW L{dW, dB, nullptr, nullptr, nullptr, nullptr, N, K};
  LinCall call{.in = {dA, lda, a_bstride}, .C = dC + c_off, .ldc = ldc, .c_bs = c_bstride, .res = dR, .ldr = ldr,
               .r_bs = r_bstride, .M = M, .batch = batch, .act = act, .trans = trans != 0, .head_rows = head_rows,
               .n_layers = n_layers, .w_ls = (int64_t)N * K, .b_ls = bias ? N : 0, .c_ls = c_lstride};
  if (use_int8) {
    int8_t* dWq;
    float* dWs;
    const LNW ln{dG, dLb};
    if ((rc = upload_quant_w(db, W, N, K, [&](int n, int k) { return (size_t)n * K + k; }, &dWq, &dWs)) ||
        (rc = quantise_rows(m, dA, ln_g ? &ln : nullptr, (int64_t)batch * M, K, nullptr, m->ws_xq)))
      return rc;
    L.wq = dWq; L.wscale = dWs;
    call.in = {.xq = &m->ws_xq};
  }
  rc = run_linear(m, L, call);
  return rc ? rc : download_f16(m->stream, C, dC, (size_t)c_elems);
}

// q,k,v,out: float32 [B][T][H*64]
int32_t fw_test_attention(fw_model* fm, const float* q, const float* k, const float* v, int32_t B, int32_t H,
                          int32_t T, float* out) {
  FW_CHECK_ARG(fm && q && k && v && out, "null argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const int d = H * 64, tp = (T + 63) / 64 * 64;
  const size_t n = (size_t)B * T * d;
  std::vector<float> vt((size_t)B * d * tp, 0.f);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int c = 0; c < d; ++c) vt[((size_t)b * d + c) * tp + t] = v[((size_t)b * T + t) * d + c];
  HookBufs db;
  half_t *dq, *dk, *dvt, *dout;
  int rc;
  if ((rc = db.upload_f16(&dq, q, n)) || (rc = db.upload_f16(&dk, k, n)) || (rc = db.upload_f16(&dvt, vt.data(), vt.size())) ||
      (rc = db.alloc(&dout, n)))
    return rc;
  fwk::launch_attn_enc(m->stream, {.q = dq, .k = dk, .ld = d, .qk_bstride = (int64_t)T * d, .vt = dvt, .ldvt = tp,
                                   .vt_bstride = (int64_t)d * tp, .out = dout, .ldo = d, .o_bstride = (int64_t)T * d,
                                   .B = B, .H = H, .T = T});
  return download_f16(m->stream, out, dout, n);
}

// measurement hook (profiles/attn_bench.py): mean milliseconds of one launch of the encoder self-attention on
// device-resident pseudo-random Q | K ([B][T][2d] as the fused projection leaves them) and V^T ([B][d][T padded]);
// variant: the workgroup -> (chunk, head, query tile) mapping (attn_enc.hip: 0 = XCD-aware, 1 = round 3's)
int32_t fw_bench_attention(fw_model* fm, int32_t B, int32_t H, int32_t T, int32_t variant, int32_t iters, float* ms_out) {
  FW_CHECK_ARG(fm && ms_out && B > 0 && H > 0 && T > 0 && iters > 0, "bad argument");
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  const int d = H * 64, tp = (T + 63) / 64 * 64;
  const size_t nqk = (size_t)B * T * 2 * d, nvt = (size_t)B * d * tp, no = (size_t)B * T * d;
  HookBufs db;
  half_t *dqk, *dvt, *dout;
  std::vector<uint16_t> stage;
  int rc;
  if ((rc = db.alloc(&dqk, nqk)) || (rc = db.alloc(&dvt, nvt)) || (rc = db.alloc(&dout, no)) ||
      (rc = fill_lcg(dqk, nqk, stage, 777u, 2e-3f)) || (rc = fill_lcg(dvt, nvt, stage, 777u, 2e-3f)))
    return rc;
  float ms = 0.f;
  const fwk::AttnEnc att{.q = dqk, .k = dqk + d, .ld = 2 * d, .qk_bstride = (int64_t)T * 2 * d, .vt = dvt, .ldvt = tp,
                         .vt_bstride = (int64_t)d * tp, .out = dout, .ldo = d, .o_bstride = (int64_t)T * d,
                         .B = B, .H = H, .T = T, .order = variant};
  rc = time_launches(m->stream, 1, iters, [&](int) { fwk::launch_attn_enc(m->stream, att); return 0; }, &ms);
  if (rc) return rc;
  *ms_out = ms / (float)iters;
  return FW_OK;
}

// ---------------------------------------------------------------- decoder attention hooks (tests/test_gpu_dec_attention.py)
// Each one uploads host buffers, runs the product's own launcher on m->stream (the form / register cap a decode step
// would take under knobs 2 / 7) and downloads.  Every index the kernels turn into an address is checked here first.
int32_t fw_test_dec_self_attn(fw_model* fm, const float* qkv, float* kcache, float* vcache, const uint8_t* kvidx,
                              int32_t n_chunks, int32_t kmul, int32_t Kbeam, int32_t H, int32_t n_ctx, int32_t cache_ctx,
                              int32_t pos_fixed, int32_t P, int32_t step, int32_t blk_n, int32_t frag, float* out) {
  FW_CHECK_ARG(fm && qkv && kcache && vcache && kvidx && out, "null argument");
  FW_CHECK_ARG(n_chunks >= 1 && H >= 1 && kmul >= 1 && kmul <= 16 && Kbeam >= 1 && Kbeam <= 255, "bad geometry");
  FW_CHECK_ARG(n_ctx >= 1 && n_ctx <= 448 && cache_ctx >= 1 && cache_ctx <= n_ctx, "need 1 <= cache_ctx <= n_ctx <= 448");
  FW_CHECK_ARG(blk_n >= 0 && (blk_n == 0 ? kmul <= Kbeam : (kmul == blk_n && pos_fixed >= 0)),
               "blk_n = 0: kmul <= Kbeam; blk_n > 0: kmul == blk_n and pos_fixed >= 0");
  const int pos0 = pos_fixed >= 0 ? pos_fixed : P - 1 + step;
  const int pos_last = pos0 + (blk_n > 0 ? blk_n - 1 : 0);
  FW_CHECK_ARG(pos0 >= 0 && pos_last < cache_ctx, "positions %d..%d outside the cache (%d)", pos0, pos_last, cache_ctx);
  const int d = H * 64, R = n_chunks * kmul, R16 = (R + 15) / 16 * 16, R_total = n_chunks * Kbeam;
  FW_CHECK_ARG(blk_n == 0 || fwd::self_attn_block_ok(n_ctx, cache_ctx, d, R_total), "position blocks need n_ctx %% 4 == 0");
  const size_t n_tab = (size_t)2 * R_total * n_ctx, n_cache = (size_t)R_total * H * cache_ctx * 64;
  for (size_t i = 0; i < n_tab; ++i)
    FW_CHECK_ARG(kvidx[i] < Kbeam, "kvidx[%zu] = %d is not a beam of %d", i, (int)kvidx[i], Kbeam);
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  HookBufs db;
  half_t *d_qkv, *d_kc, *d_vc, *d_out;
  uint8_t* d_idx;
  int* d_step;
  int rc;
  if ((rc = db.upload_f16(&d_qkv, qkv, (size_t)R * 3 * d)) || (rc = db.upload_f16(&d_kc, kcache, n_cache)) ||
      (rc = db.upload_f16(&d_vc, vcache, n_cache)) || (rc = db.alloc(&d_out, (size_t)R16 * d)) ||
      (rc = db.upload(&d_idx, kvidx, n_tab)) || (rc = db.upload(&d_step, &step, 1)) ||
      (rc = db.zero(d_out, (size_t)R16 * d * 2, st)))
    return rc;
  fwd::launch_self_attn(st, d_qkv, d, d_kc, d_vc, n_ctx, cache_ctx, H, d_idx, Kbeam, kmul, d_out, R, d_step, pos_fixed, P,
                        R_total, frag ? 1 : 0, blk_n);
  FW_HIP(hipGetLastError());
  if ((rc = download_f16(st, kcache, d_kc, n_cache)) || (rc = download_f16(st, vcache, d_vc, n_cache))) return rc;
  return frag ? download_f16_frag(st, out, d_out, R, d) : download_f16(st, out, d_out, (size_t)R * d);
}

int32_t fw_test_dec_cross_attn(fw_model* fm, const float* q, const float* k, const float* v, int32_t n_enc, int32_t T,
                               int32_t H, int32_t B, int32_t kmul, int32_t kv_div, const int32_t* slot_map,
                               const int32_t* done, int32_t frag, float k_pad, float* out) {
  FW_CHECK_ARG(fm && q && k && v && slot_map && out, "null argument");
  FW_CHECK_ARG(n_enc >= 1 && T >= 1 && H >= 1 && B >= 1 && kmul >= 1 && kmul <= 16 && kv_div >= 1, "bad geometry");
  const int n_map = (B + kv_div - 1) / kv_div;
  for (int i = 0; i < n_map; ++i)
    FW_CHECK_ARG(slot_map[i] >= 0 && slot_map[i] < n_enc, "slot_map[%d] = %d outside [0, %d)", i, slot_map[i], n_enc);
  const int d = H * 64, kvp = (T + 31) / 32 * 32, R = B * kmul, R16 = (R + 15) / 16 * 16;
  const size_t blk = (size_t)d * kvp;   // one encoder chunk's K (or V^T)
  // the pool's layout and contract (decoder.hip: CrossPool): padded keys of K hold whatever (k_pad), of V^T zeros
  std::vector<float> kf((size_t)n_enc * blk), vf((size_t)n_enc * blk, 0.f);
  for (int e = 0; e < n_enc; ++e)
    for (int t = 0; t < kvp; ++t)
      for (int n = 0; n < d; ++n) {
        const size_t src = ((size_t)e * T + t) * d + n;
        kf[e * blk + cross_kv_frag_pos(false, kvp, t, n)] = t < T ? k[src] : k_pad;
        if (t < T) vf[e * blk + cross_kv_frag_pos(true, kvp, t, n)] = v[src];
      }
  std::vector<float> of((size_t)R16 * d, 0.f);   // the output as the device holds it: whole 16-row tiles
  for (int r = 0; r < R; ++r)
    for (int n = 0; n < d; ++n) of[frag ? frag_pos(r, n, d, 32) : (size_t)r * d + n] = out[(size_t)r * d + n];
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  half_t *d_q, *d_k, *d_vt, *d_out;
  int *d_map, *d_done = nullptr;
  int rc;
  if ((rc = db.upload_f16(&d_q, q, (size_t)R * d)) || (rc = db.upload_f16(&d_k, kf.data(), kf.size())) ||
      (rc = db.upload_f16(&d_vt, vf.data(), vf.size())) || (rc = db.upload_f16(&d_out, of.data(), of.size())) ||
      (rc = db.upload(&d_map, slot_map, (size_t)n_map)) || (done && (rc = db.upload(&d_done, done, (size_t)B))))
    return rc;
  fwd::launch_cross_attn(m->stream, d_q, d, d_k, d_vt, T, kvp, kmul, d_out, B, H, d_done, kv_div, frag ? 1 : 0, d_map);
  FW_HIP(hipGetLastError());
  return frag ? download_f16_frag(m->stream, out, d_out, R, d) : download_f16(m->stream, out, d_out, (size_t)R * d);
}

int32_t fw_test_dec_cross_probs(fw_model* fm, const float* q, const float* k, int32_t B, int32_t T, int32_t H,
                                const int32_t* heads, int32_t n_sel, int32_t n_tok, int32_t tok_idx, int32_t blk_n,
                                float* probs) {
  FW_CHECK_ARG(fm && q && k && heads && probs, "null argument");
  const int blk = blk_n > 0 ? blk_n : 1;
  FW_CHECK_ARG(B >= 1 && T >= 1 && H >= 1 && n_sel >= 1 && blk_n >= 0 && blk <= 16, "bad geometry");
  FW_CHECK_ARG(tok_idx >= 0 && tok_idx + blk <= n_tok, "tokens %d..%d outside [0, %d)", tok_idx, tok_idx + blk - 1, n_tok);
  for (int i = 0; i < n_sel; ++i) FW_CHECK_ARG(heads[i] >= 0 && heads[i] < H, "heads[%d] = %d outside [0, %d)", i, heads[i], H);
  const int d = H * 64, kvp = (T + 31) / 32 * 32;
  const size_t blkk = (size_t)d * kvp, n_probs = (size_t)B * n_sel * n_tok * T;
  std::vector<float> kf((size_t)B * blkk, 0.f);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int n = 0; n < d; ++n) kf[b * blkk + cross_kv_frag_pos(false, kvp, t, n)] = k[((size_t)b * T + t) * d + n];
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  half_t *d_q, *d_k;
  int* d_heads;
  float* d_p;
  int rc;
  if ((rc = db.upload_f16(&d_q, q, (size_t)B * blk * d)) || (rc = db.upload_f16(&d_k, kf.data(), kf.size())) ||
      (rc = db.upload(&d_heads, heads, (size_t)n_sel)) || (rc = db.upload(&d_p, probs, n_probs)))
    return rc;
  fwd::launch_cross_probs(m->stream, d_q, d, d_k, T, kvp, d_heads, n_sel, n_sel, d_p, n_tok, tok_idx, B, blk_n);
  FW_HIP(hipGetLastError());
  FW_HIP(hipStreamSynchronize(m->stream));
  return download(probs, d_p, n_probs);
}

int32_t fw_test_dec_softmax_pick(fw_model* fm, const float* logits, int32_t rows, int32_t V, int32_t row_mul,
                                 const int32_t* target, int32_t nospeech, float* out) {
  FW_CHECK_ARG(fm && logits && target && out, "null argument");
  FW_CHECK_ARG(rows >= 1 && V >= 1 && row_mul >= 1, "bad geometry");
  FW_CHECK_ARG(!nospeech || (target[0] >= 0 && target[0] < V), "no-speech id %d outside [0, %d)", target[0], V);
  Model* m = &fm->impl;
  std::lock_guard<std::mutex> lk(m->mu);
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  const size_t n_lg = (size_t)rows * row_mul * V;
  float *d_lg, *d_out;
  int* d_t;
  int rc;
  if ((rc = db.upload(&d_lg, logits, n_lg)) || (rc = db.alloc(&d_out, (size_t)rows)) || (rc = db.alloc(&d_t, (size_t)rows))) return rc;
  FW_HIP(hipMemcpy(d_t, target, (size_t)(nospeech ? 1 : rows) * sizeof(int), hipMemcpyHostToDevice));
  if (nospeech) fwd::launch_nospeech(m->stream, d_lg, V, row_mul, target[0], d_out, rows);
  else fwd::launch_token_prob(m->stream, d_lg, V, d_t, d_out, 1, 0, rows, row_mul);
  FW_HIP(hipGetLastError());
  FW_HIP(hipStreamSynchronize(m->stream));
  return download(out, d_out, (size_t)rows);
}

// ---------------------------------------------------------------------------------------------------
// Test hook: ONE launch of the logits-rules kernel (rules, log-softmax, top-2K / Gumbel arg-max) on caller-provided
// logits and row state, outside any decode run: tests/test_gpu_logits_rules.py compares the candidates with the
// oracle's rule restatement id for id.  rows = R (row r belongs to chunk r / beam_size), n = tokens generated so far
// (the same for every row), hist [R][n], cum [R]; out: cand_val / cand_tok [R][2 * beam_size] (sampling: [R][1]).
// (This hook and the four after it launch on the null stream, without the model's lock, and end with a device-wide wait.)
// ---------------------------------------------------------------------------------------------------
// (cand_lp null: the kernel gets a null pointer and skips the log-prob stores, fw_test_logits_rules as it always was)
// smp: the sampling table of the launch, one entry per row (fw_test_logits_rules_smp_tab); null: every row is a row of ONE
// call with the temperature and seed of `o` (row0 = 0), what a decode run of that call alone fills in
// ex (fw_test_logits_rules_ex): the state exposed.  done [R / K] | null (all live); the logits rows are downloaded whole
// into logits_io after the launch; cand_val / cand_tok / cand_lp are [R][32], the kernel's own stride, IN / OUT: the device
// buffers start as the caller's values and come back whole.  Without it the outputs start as zeros and the first C columns
// of every row are returned.
// Every history id is checked in [0, V) before anything is allocated or launched: the repetition penalty and the n-gram
// rule use them as indices into the row (a wrong test gets FW_EINVAL, never a device fault).
// alt (fw_test_logits_rules_alt): n_alt in [1, FW_MAX_ALTERNATIVES] and alt_tok / alt_lp [R][n_alt] IN / OUT — the rows' slab
// [n][.][.] of a step-major device buffer of n + 1 steps, which is what the kernel indexes with its step counter.
// trunc (fw_test_logits_rules_trunc): top_k / top_p [R], the launch's TruncRow table; the launch is then ONE launch of the
// TRUNC instantiation (gp.trunc = 1) whatever the rows' limits are.
struct RulesEx {
  const int32_t* done; float* logits_io; int32_t n_alt = 0; int32_t* alt_tok = nullptr; float* alt_lp = nullptr;
  const int32_t* top_k = nullptr; const float* top_p = nullptr;
};
static int32_t logits_rules_hook(fw_model* fm, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                                 const float* cum, const fw_gen_opts* o, int32_t with_timestamps, float* cand_val,
                                 int32_t* cand_tok, float* cand_lp, const fwd::SmpRow* smp = nullptr,
                                 const RulesEx* ex = nullptr) {
  FW_CHECK_ARG(fm && logits && cum && o && cand_val && cand_tok && R >= 1 && n >= 0, "bad arguments");
  Model* m = &fm->impl;
  const fw_config& c = m->cfg;
  const int K = o->beam_size;
  const bool sampling = K == 1 && o->sampling_topk != 1;
  FW_CHECK_ARG(K >= 1 && K <= 16 && R % K == 0 && n < c.n_text_ctx && (n == 0 || hist), "bad geometry");
  FW_CHECK_ARG(c.n_vocab <= LP_SUP_WORDS * 64, "vocabulary too large for the rules kernel");
  for (size_t i = 0; i < (size_t)R * n; ++i)
    FW_CHECK_ARG(hist[i] >= 0 && hist[i] < c.n_vocab, "hist[%d][%d] = %d outside [0, %d)", (int)(i / n), (int)(i % n),
                 hist[i], c.n_vocab);
  if (ex && ex->done)
    for (int b = 0; b < R / K; ++b) FW_CHECK_ARG(ex->done[b] == 0 || ex->done[b] == 1, "done[%d] = %d is not 0 / 1", b, ex->done[b]);
  const int n_alt = ex ? ex->n_alt : 0;
  FW_CHECK_ARG(n_alt >= 0 && n_alt <= FW_MAX_ALTERNATIVES, "n_alt %d not in [0, %d]", n_alt, FW_MAX_ALTERNATIVES);
  FW_HIP(hipSetDevice(m->device));
  GenDev gp;
  memset(&gp, 0, sizeof(gp));
  gp.B = R / K; gp.K = K; gp.R = R; gp.V = c.n_vocab; gp.n_text_ctx = c.n_text_ctx;
  gp.n_alt = n_alt;
  gp.sample = sampling ? 1 : 0;
  const bool trunc = ex && ex->top_k && ex->top_p;
  FW_CHECK_ARG(!trunc || sampling, "truncation needs options that select sampling");
  if (trunc)
    for (int r = 0; r < R; ++r)
      FW_CHECK_ARG(ex->top_k[r] >= 0 && ex->top_p[r] > 0.f && ex->top_p[r] <= 1.f, "row %d: top_k %d / top_p %g out of range",
                   r, ex->top_k[r], (double)ex->top_p[r]);
  gp.trunc = trunc ? 1 : 0;
  gp.inv_temp = 1.0f;   // (sampling: temperature and seed per row, from the table below — as in a decode run)
  fwd::fill_rule_fields(gp, c, o, with_timestamps);
  const std::vector<unsigned long long> mask = fwd::suppress_mask(o->suppress_tokens, o->n_suppress_tokens, c.n_vocab);
  const size_t NT = (size_t)c.n_text_ctx;
  std::vector<int> h2(2 * (size_t)R * NT, 0);
  std::vector<float> c2(2 * (size_t)R, 0.f);
  const int cur = n & 1;   // the kernel reads the half selected by the step's parity
  for (int r = 0; r < R; ++r) {
    for (int i = 0; i < n; ++i) h2[((size_t)cur * R + r) * NT + i] = hist[(size_t)r * n + i];
    c2[(size_t)cur * R + r] = cum[r];
  }
  std::vector<int> dn((size_t)R, 0);   // (the kernel reads done[r / K]; R entries as the hook always allocated)
  if (ex && ex->done) std::copy(ex->done, ex->done + R / K, dn.begin());
  const size_t NC = (size_t)R * 32;
  std::vector<float> hv(NC, 0.f), hl(cand_lp ? NC : 0, 0.f);
  std::vector<int> ht(NC, 0);
  if (ex) {
    std::copy(cand_val, cand_val + NC, hv.begin());
    std::copy(cand_tok, cand_tok + NC, ht.begin());
    if (cand_lp) std::copy(cand_lp, cand_lp + NC, hl.begin());
  }
  HookBufs db;
  float *d_lg, *d_cum, *d_cv, *d_cl = nullptr;
  int *d_hist, *d_step, *d_done, *d_ct;
  unsigned long long* d_bits;
  int rc;
  if ((rc = db.upload(&d_lg, logits, (size_t)R * c.n_vocab)) || (rc = db.upload(&d_cum, c2.data(), c2.size())) ||
      (rc = db.upload(&d_hist, h2.data(), h2.size())) || (rc = db.upload(&d_step, &n, 1)) ||
      (rc = db.upload(&d_bits, mask.data(), mask.size())) || (rc = db.upload(&d_done, dn.data(), dn.size())) ||
      (rc = db.upload(&d_cv, hv.data(), NC)) || (rc = db.upload(&d_ct, ht.data(), NC)))
    return rc;
  if (cand_lp && (rc = db.upload(&d_cl, hl.data(), NC))) return rc;
  fwd::SmpRow* d_smp = nullptr;
  if (sampling) {
    std::vector<fwd::SmpRow> tab((size_t)R);
    for (int r = 0; r < R; ++r)
      tab[r] = smp ? smp[r]
                   : fwd::SmpRow{1.0f / o->sampling_temperature, (unsigned)(o->seed & 0xffffffffu), (unsigned)(o->seed >> 32), 0};
    if ((rc = db.upload(&d_smp, tab.data(), tab.size()))) return rc;
  }
  int* d_at = nullptr;
  float* d_al = nullptr;
  const size_t n_slab = (size_t)R * n_alt;   // the slab of step n; the steps before it are never touched
  if (n_alt > 0) {
    if ((rc = db.alloc(&d_at, (size_t)(n + 1) * n_slab)) || (rc = db.alloc(&d_al, (size_t)(n + 1) * n_slab))) return rc;
    FW_HIP(hipMemcpy(d_at + (size_t)n * n_slab, ex->alt_tok, n_slab * sizeof(int), hipMemcpyHostToDevice));
    FW_HIP(hipMemcpy(d_al + (size_t)n * n_slab, ex->alt_lp, n_slab * sizeof(float), hipMemcpyHostToDevice));
  }
  fwd::TruncRow* d_trunc = nullptr;
  if (trunc) {
    std::vector<fwd::TruncRow> tab((size_t)R);
    for (int r = 0; r < R; ++r) tab[r] = {ex->top_k[r], ex->top_p[r]};
    if ((rc = db.upload(&d_trunc, tab.data(), tab.size()))) return rc;
  }
  fwd::launch_logits_process(nullptr, gp, d_lg, d_bits, d_hist, d_cum, d_step, d_done, d_cv, d_ct, d_cl, d_smp, d_at, d_al,
                             d_trunc);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  if ((rc = download(hv.data(), d_cv, NC)) || (rc = download(ht.data(), d_ct, NC))) return rc;
  if (n_alt > 0 && ((rc = download(ex->alt_tok, d_at + (size_t)n * n_slab, n_slab)) ||
                    (rc = download(ex->alt_lp, d_al + (size_t)n * n_slab, n_slab))))
    return rc;
  if (cand_lp && (rc = download(hl.data(), d_cl, NC))) return rc;
  if (ex && ex->logits_io && (rc = download(ex->logits_io, d_lg, (size_t)R * c.n_vocab))) return rc;
  const int C = ex ? 32 : sampling ? 1 : 2 * K;
  for (int r = 0; r < R; ++r)
    for (int j = 0; j < C; ++j) {
      cand_val[(size_t)r * C + j] = hv[(size_t)r * 32 + j];
      cand_tok[(size_t)r * C + j] = ht[(size_t)r * 32 + j];
      if (cand_lp) cand_lp[(size_t)r * C + j] = hl[(size_t)r * 32 + j];
    }
  return FW_OK;
}

int32_t fw_test_logits_rules(fw_model* fm, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                             const float* cum, const fw_gen_opts* o, int32_t with_timestamps, float* cand_val,
                             int32_t* cand_tok) {
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, nullptr);
}

int32_t fw_test_logits_rules_lp(fw_model* fm, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                                const float* cum, const fw_gen_opts* o, int32_t with_timestamps, float* cand_val,
                                int32_t* cand_tok, float* cand_lp) {
  FW_CHECK_ARG(cand_lp, "null argument");
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, cand_lp);
}

// the sampling table of a launch from the per-row arrays of the C ABI (row0[r] in [0, r], inv_temp[r] > 0: checked)
static int32_t smp_table(int32_t R, const float* inv_temp, const uint64_t* seed, const int32_t* row0,
                         std::vector<fwd::SmpRow>& tab) {
  tab.resize((size_t)R);
  for (int r = 0; r < R; ++r) {
    FW_CHECK_ARG(row0[r] >= 0 && row0[r] <= r && inv_temp[r] > 0.f, "row %d: row0 must lie in [0, row], inv_temp must be positive", r);
    tab[r] = {inv_temp[r], (unsigned)(seed[r] & 0xffffffffu), (unsigned)(seed[r] >> 32), row0[r]};
  }
  return FW_OK;
}

// The sampling instantiation over R rows that belong to DIFFERENT calls, as in a merged sampling run: row r draws with
// 1 / inv_temp[r] as its temperature and seed[r], as row r - row0[r] of its call (0 <= row0[r] <= r: checked).  `o` gives the
// rules and must select sampling (beam_size 1, sampling_topk 0); its own temperature and seed are not read.
int32_t fw_test_logits_rules_smp_tab(fw_model* fm, const float* logits, int32_t R, const int32_t* hist, int32_t n,
                                     const float* cum, const fw_gen_opts* o, int32_t with_timestamps,
                                     const float* inv_temp, const uint64_t* seed, const int32_t* row0, float* cand_val,
                                     int32_t* cand_tok, float* cand_lp) {
  FW_CHECK_ARG(o && inv_temp && seed && row0 && cand_lp && R >= 1, "null argument");
  FW_CHECK_ARG(o->beam_size == 1 && o->sampling_topk == 0, "the options must select sampling (beam_size 1, sampling_topk 0)");
  std::vector<fwd::SmpRow> tab;
  if (int rc = smp_table(R, inv_temp, seed, row0, tab)) return rc;
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, cand_lp, tab.data());
}

// fw_test_logits_rules_lp with the state exposed (include/fwamd_test.h): logits IN / OUT, done per chunk, candidate arrays
// [R][32] IN / OUT, the sampling table of fw_test_logits_rules_smp_tab or none.
int32_t fw_test_logits_rules_ex(fw_model* fm, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                const fw_gen_opts* o, int32_t with_timestamps, const int32_t* done, const float* inv_temp,
                                const uint64_t* seed, const int32_t* row0, float* cand_val, int32_t* cand_tok,
                                float* cand_lp) {
  FW_CHECK_ARG(o && cand_lp && R >= 1, "null argument");
  const bool tab_given = inv_temp || seed || row0;
  FW_CHECK_ARG(!tab_given || (inv_temp && seed && row0), "the sampling table needs inv_temp, seed and row0 together");
  std::vector<fwd::SmpRow> tab;
  if (tab_given) {
    FW_CHECK_ARG(o->beam_size == 1 && o->sampling_topk == 0, "the options must select sampling (beam_size 1, sampling_topk 0)");
    if (int rc = smp_table(R, inv_temp, seed, row0, tab)) return rc;
  }
  const RulesEx ex{done, logits};
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, cand_lp,
                           tab_given ? tab.data() : nullptr, &ex);
}

// fw_test_logits_rules_ex plus alternatives (include/fwamd_test.h): the ALT instantiations of the rules kernel.
int32_t fw_test_logits_rules_alt(fw_model* fm, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                 const fw_gen_opts* o, int32_t with_timestamps, const int32_t* done, const float* inv_temp,
                                 const uint64_t* seed, const int32_t* row0, float* cand_val, int32_t* cand_tok,
                                 float* cand_lp, int32_t n_alt, int32_t* alt_tok, float* alt_lp) {
  FW_CHECK_ARG(o && cand_lp && alt_tok && alt_lp && R >= 1, "null argument");
  FW_CHECK_ARG(n_alt >= 1 && n_alt <= FW_MAX_ALTERNATIVES, "n_alt %d not in [1, %d]", n_alt, FW_MAX_ALTERNATIVES);
  const bool tab_given = inv_temp || seed || row0;
  FW_CHECK_ARG(!tab_given || (inv_temp && seed && row0), "the sampling table needs inv_temp, seed and row0 together");
  std::vector<fwd::SmpRow> tab;
  if (tab_given) {
    FW_CHECK_ARG(o->beam_size == 1 && o->sampling_topk == 0, "the options must select sampling (beam_size 1, sampling_topk 0)");
    if (int rc = smp_table(R, inv_temp, seed, row0, tab)) return rc;
  }
  const RulesEx ex{done, logits, n_alt, alt_tok, alt_lp};
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, cand_lp,
                           tab_given ? tab.data() : nullptr, &ex);
}

// fw_test_logits_rules_alt plus per-row limits (include/fwamd_test.h): ONE launch of the TRUNC instantiation; n_alt may be 0.
int32_t fw_test_logits_rules_trunc(fw_model* fm, float* logits, int32_t R, const int32_t* hist, int32_t n, const float* cum,
                                   const fw_gen_opts* o, int32_t with_timestamps, const int32_t* done, const float* inv_temp,
                                   const uint64_t* seed, const int32_t* row0, const int32_t* top_k, const float* top_p,
                                   float* cand_val, int32_t* cand_tok, float* cand_lp, int32_t n_alt, int32_t* alt_tok,
                                   float* alt_lp) {
  FW_CHECK_ARG(o && cand_lp && top_k && top_p && R >= 1, "null argument");
  FW_CHECK_ARG(n_alt >= 0 && n_alt <= FW_MAX_ALTERNATIVES, "n_alt %d not in [0, %d]", n_alt, FW_MAX_ALTERNATIVES);
  FW_CHECK_ARG(n_alt == 0 ? (!alt_tok && !alt_lp) : (alt_tok && alt_lp), "alt_tok / alt_lp: both with n_alt > 0, none with n_alt == 0");
  FW_CHECK_ARG(o->beam_size == 1 && o->sampling_topk == 0, "the options must select sampling (beam_size 1, sampling_topk 0)");
  const bool tab_given = inv_temp || seed || row0;
  FW_CHECK_ARG(!tab_given || (inv_temp && seed && row0), "the sampling table needs inv_temp, seed and row0 together");
  std::vector<fwd::SmpRow> tab;
  if (tab_given)
    if (int rc = smp_table(R, inv_temp, seed, row0, tab)) return rc;
  const RulesEx ex{done, logits, n_alt, alt_tok, alt_lp, top_k, top_p};
  return logits_rules_hook(fm, logits, R, hist, n, cum, o, with_timestamps, cand_val, cand_tok, cand_lp,
                           tab_given ? tab.data() : nullptr, &ex);
}

// ONE launch of the scoring kernel on caller-provided rows (include/fwamd_test.h): row r is scored against targets[r] with
// the history hist[hist_offsets[r] .. hist_offsets[r + 1]); opts null: the raw distribution.  Every id is checked before
// anything is allocated or launched: the sparse rules and the target pick index the row with them.
int32_t fw_test_score_rows(fw_model* fm, float* logits, int32_t rows, const int32_t* targets, const int32_t* hist,
                           const int32_t* hist_offsets, const fw_gen_opts* o, int32_t with_timestamps, float* out_lp,
                           int32_t* out_best_id, float* out_best_lp) {
  FW_CHECK_ARG(fm && logits && targets && hist_offsets && out_lp && out_best_id && out_best_lp && rows >= 1, "bad arguments");
  Model* m = &fm->impl;
  const fw_config& c = m->cfg;
  FW_CHECK_ARG(c.n_vocab <= LP_SUP_WORDS * 64 && c.n_text_ctx <= 1024, "model too large for the scoring kernel");
  FW_CHECK_ARG(hist_offsets[0] == 0, "hist_offsets must start at 0");
  std::vector<fwd::ScoreRow> tab((size_t)rows);
  for (int r = 0; r < rows; ++r) {
    const int n = hist_offsets[r + 1] - hist_offsets[r];
    FW_CHECK_ARG(n >= 0 && n < c.n_text_ctx && (n == 0 || hist), "row %d: a history of %d ids (text context %d)", r, n, c.n_text_ctx);
    FW_CHECK_ARG(targets[r] < c.n_vocab, "targets[%d] = %d outside [0, %d)", r, targets[r], c.n_vocab);
    for (int i = 0; i < n; ++i) {
      const int t = hist[hist_offsets[r] + i];
      FW_CHECK_ARG(t >= 0 && t < c.n_vocab, "hist of row %d, entry %d = %d outside [0, %d)", r, i, t, c.n_vocab);
    }
    tab[r] = {targets[r], n, hist_offsets[r], r};
  }
  FW_HIP(hipSetDevice(m->device));
  GenDev gp;
  memset(&gp, 0, sizeof(gp));
  gp.B = rows; gp.K = 1; gp.R = rows; gp.V = c.n_vocab; gp.n_text_ctx = c.n_text_ctx; gp.kv_div = 1;
  fwd::fill_rule_fields(gp, c, o, with_timestamps);
  gp.min_new = 0;   // as fw_score: min_new_tokens is not a rule of scoring
  const std::vector<unsigned long long> mask = fwd::suppress_mask(o ? o->suppress_tokens : nullptr, o ? o->n_suppress_tokens : 0, c.n_vocab);
  const size_t n_hist = (size_t)hist_offsets[rows];
  const int zero = 0;
  HookBufs db;
  float *d_lg, *d_lp, *d_blp;
  int *d_hist, *d_bid;
  fwd::ScoreRow* d_tab;
  unsigned long long* d_bits;
  int rc;
  if ((rc = db.upload(&d_lg, (const float*)logits, (size_t)rows * c.n_vocab)) || (rc = db.upload(&d_tab, tab.data(), tab.size())) ||
      (rc = db.upload(&d_hist, n_hist ? hist : &zero, std::max<size_t>(1, n_hist))) ||
      (rc = db.upload(&d_bits, mask.data(), mask.size())) || (rc = db.upload(&d_lp, (const float*)out_lp, (size_t)rows)) ||
      (rc = db.upload(&d_bid, (const int*)out_best_id, (size_t)rows)) || (rc = db.upload(&d_blp, (const float*)out_best_lp, (size_t)rows)))
    return rc;
  fwd::launch_score(nullptr, gp, o != nullptr, d_lg, d_bits, d_tab, 1, 0, 1, rows, d_hist, d_lp, d_bid, d_blp);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  if ((rc = download(out_lp, d_lp, (size_t)rows)) || (rc = download(out_best_id, d_bid, (size_t)rows)) ||
      (rc = download(out_best_lp, d_blp, (size_t)rows)))
    return rc;
  return download(logits, d_lg, (size_t)rows * c.n_vocab);
}

// the histories of a boost hook: offsets from 0, non-decreasing, every n below `n_limit` (< 0: no limit), every id in [0, V)
static int32_t boost_hist_check(int32_t rows, const int32_t* hist, const int32_t* hist_offsets, int n_limit, int V) {
  FW_CHECK_ARG(hist_offsets[0] == 0, "hist_offsets must start at 0");
  for (int r = 0; r < rows; ++r) {
    const int64_t n = (int64_t)hist_offsets[r + 1] - hist_offsets[r];
    FW_CHECK_ARG(n >= 0 && (n_limit < 0 || n < n_limit) && (n == 0 || hist), "row %d: a history of %lld ids", r, (long long)n);
    for (int i = 0; i < n; ++i) {
      const int t = hist[hist_offsets[r] + i];
      FW_CHECK_ARG(t >= 0 && t < V, "hist of row %d, entry %d = %d outside [0, %d)", r, i, t, V);
    }
  }
  return FW_OK;
}

// What fw_test_boost_rows and fw_test_constrain_rows do alike: ONE launch of a pre-pass kernel in either row form
// (include/fwamd_test.h) over `rows` rows of gp.V logits.  gp holds what the kernel reads beyond the rows (the callers have
// checked it and the list); B, K and R are set here.  Everything is checked before anything is allocated or launched.
using PrepassStep = void (*)(hipStream_t, const GenDev&, float*, const int*, const int*, const int*, const int*);
using PrepassScore = void (*)(hipStream_t, const GenDev&, float*, const int*, const fwd::ScoreRow*, int, int, int, int, const int*);
static int32_t prepass_rows(Model* m, GenDev gp, float* logits, int32_t rows, const int32_t* hist, const int32_t* hist_offsets,
                            int32_t K, const int32_t* done, int32_t form, const std::vector<int32_t>& table,
                            PrepassStep launch_step, PrepassScore launch_score) {
  FW_CHECK_ARG(form == 0 ? (K >= 1 && K <= 16 && rows % K == 0) : K == 1, "bad K %d for form %d and %d rows", K, form, rows);
  if (int rc = boost_hist_check(rows, hist, hist_offsets, gp.n_text_ctx, gp.V)) return rc;
  const int n0 = hist_offsets[1];
  if (form == 0)
    for (int r = 0; r < rows; ++r)
      FW_CHECK_ARG(hist_offsets[r + 1] - hist_offsets[r] == n0, "form 0 takes one n for all rows (row %d)", r);
  const int n_done = form == 0 ? rows / K : rows;
  if (done)
    for (int b = 0; b < n_done; ++b) FW_CHECK_ARG(done[b] == 0 || done[b] == 1, "done[%d] = %d is not 0 / 1", b, done[b]);
  FW_HIP(hipSetDevice(m->device));
  gp.B = rows / K; gp.K = K; gp.R = rows;
  HookBufs db;
  float* d_lg;
  int* d_tab;
  int rc;
  if ((rc = db.upload(&d_lg, (const float*)logits, (size_t)rows * gp.V)) ||
      (rc = db.upload(&d_tab, (const int*)table.data(), table.size())))
    return rc;
  if (form == 0) {
    const size_t NT = (size_t)gp.n_text_ctx;
    std::vector<int> h2(2 * (size_t)rows * NT, 0), dn((size_t)rows, 0);
    for (int r = 0; r < rows; ++r)
      for (int i = 0; i < n0; ++i) h2[((size_t)(n0 & 1) * rows + r) * NT + i] = hist[hist_offsets[r] + i];
    if (done) std::copy(done, done + n_done, dn.begin());
    int *d_hist, *d_step, *d_done;
    if ((rc = db.upload(&d_hist, h2.data(), h2.size())) || (rc = db.upload(&d_step, &n0, 1)) ||
        (rc = db.upload(&d_done, dn.data(), dn.size())))
      return rc;
    launch_step(nullptr, gp, d_lg, d_tab, d_hist, d_step, d_done);
  } else {
    std::vector<fwd::ScoreRow> tab((size_t)rows);
    for (int r = 0; r < rows; ++r)
      tab[r] = {(done && done[r]) ? -1 : 0, hist_offsets[r + 1] - hist_offsets[r], hist_offsets[r], r};
    const size_t n_hist = (size_t)hist_offsets[rows];
    const int zero = 0;
    fwd::ScoreRow* d_rows;
    int* d_hist;
    if ((rc = db.upload(&d_rows, tab.data(), tab.size())) ||
        (rc = db.upload(&d_hist, n_hist ? hist : &zero, std::max<size_t>(1, n_hist))))
      return rc;
    launch_score(nullptr, gp, d_lg, d_tab, d_rows, 1, 0, 1, rows, d_hist);
  }
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  return download(logits, d_lg, (size_t)rows * gp.V);
}

int32_t fw_test_boost_rows(fw_model* fm, float* logits, int32_t rows, const int32_t* hist, const int32_t* hist_offsets,
                           int32_t K, const int32_t* done, int32_t form, const fw_boost* boost) {
  FW_CHECK_ARG(fm && logits && hist_offsets && boost && rows >= 1, "bad arguments");
  FW_CHECK_ARG(form == 0 || form == 1, "form %d is not 0 (decode step) / 1 (scoring)", form);
  const fw_config& c = fm->impl.cfg;
  FW_CHECK_ARG(boost->n_vocab == c.n_vocab, "the boost list was built for a vocabulary of %d ids, the model has %d",
               boost->n_vocab, c.n_vocab);
  GenDev gp;
  memset(&gp, 0, sizeof(gp));
  gp.V = c.n_vocab; gp.n_text_ctx = c.n_text_ctx; gp.kv_div = 1; gp.boost = 1;
  return prepass_rows(&fm->impl, gp, logits, rows, hist, hist_offsets, K, done, form, boost->table, fwd::launch_boost_step,
                      fwd::launch_boost_score);
}

// the same table walked on the host: no device, no model
int32_t fw_test_boost_rows_host(float* logits, int32_t rows, const int32_t* hist, const int32_t* hist_offsets,
                                const fw_boost* boost) {
  FW_CHECK_ARG(logits && hist_offsets && boost && rows >= 1, "bad arguments");
  if (int rc = boost_hist_check(rows, hist, hist_offsets, -1, boost->n_vocab)) return rc;
  const int zero = 0;
  fwd::boost_rows_host(boost->table.data(), logits, rows, boost->n_vocab, hist ? hist : &zero, hist_offsets);
  return FW_OK;
}

// what both constraint hooks check of the caller's vocabulary geometry and list
static int32_t constrain_hook_check(int32_t n_vocab, int32_t tok_eot, int32_t tok_ts_begin, int32_t with_timestamps,
                                    const fw_constraint* ct) {
  FW_CHECK_ARG(n_vocab >= 1 && n_vocab <= LP_SUP_WORDS * 64 && tok_eot >= 0 && tok_eot < tok_ts_begin && tok_ts_begin <= n_vocab,
               "bad vocabulary geometry: %d ids, <eot> %d, first timestamp %d", n_vocab, tok_eot, tok_ts_begin);
  FW_CHECK_ARG(with_timestamps == 0 || with_timestamps == 1, "with_timestamps %d is not 0 / 1", with_timestamps);
  FW_CHECK_ARG(ct->n_vocab == n_vocab, "the constraint list was built for a vocabulary of %d ids, not %d", ct->n_vocab, n_vocab);
  return FW_OK;
}

// The model gives the device and the text context (the stride of the step form's histories) only.
int32_t fw_test_constrain_rows(fw_model* fm, float* logits, int32_t rows, int32_t n_vocab, int32_t tok_eot,
                               int32_t tok_ts_begin, int32_t with_timestamps, const int32_t* hist, const int32_t* hist_offsets,
                               int32_t K, const int32_t* done, int32_t form, const fw_constraint* constraint) {
  FW_CHECK_ARG(fm && logits && hist_offsets && constraint && rows >= 1, "bad arguments");
  FW_CHECK_ARG(form == 0 || form == 1, "form %d is not 0 (decode step) / 1 (scoring)", form);
  if (int rc = constrain_hook_check(n_vocab, tok_eot, tok_ts_begin, with_timestamps, constraint)) return rc;
  GenDev gp;
  memset(&gp, 0, sizeof(gp));
  gp.V = n_vocab; gp.n_text_ctx = fm->impl.cfg.n_text_ctx; gp.kv_div = 1; gp.constrain = 1;
  gp.eot = tok_eot; gp.ts_begin = tok_ts_begin; gp.with_ts = with_timestamps;
  return prepass_rows(&fm->impl, gp, logits, rows, hist, hist_offsets, K, done, form, constraint->table,
                      fwd::launch_constrain_step, fwd::launch_constrain_score);
}

// the same table walked on the host: no device, no model
int32_t fw_test_constrain_rows_host(float* logits, int32_t rows, int32_t n_vocab, int32_t tok_eot, int32_t tok_ts_begin,
                                    int32_t with_timestamps, const int32_t* hist, const int32_t* hist_offsets,
                                    const fw_constraint* constraint) {
  FW_CHECK_ARG(logits && hist_offsets && constraint && rows >= 1, "bad arguments");
  if (int rc = constrain_hook_check(n_vocab, tok_eot, tok_ts_begin, with_timestamps, constraint)) return rc;
  if (int rc = boost_hist_check(rows, hist, hist_offsets, -1, n_vocab)) return rc;
  const int zero = 0;
  fwd::constrain_rows_host(constraint->table.data(), logits, rows, n_vocab, tok_eot, tok_ts_begin, with_timestamps,
                           hist ? hist : &zero, hist_offsets);
  return FW_OK;
}

// the compiled table of a constraint list, for the byte-equality the merge rule rests on: *out_words = its size in 32-bit
// words; `out` (may be NULL) receives min(cap, size) words
int32_t fw_test_constraint_table(const fw_constraint* constraint, int32_t* out, int32_t cap, int32_t* out_words) {
  FW_CHECK_ARG(constraint && out_words && cap >= 0 && (out || cap == 0), "bad arguments");
  *out_words = (int32_t)constraint->table.size();
  std::copy(constraint->table.begin(), constraint->table.begin() + std::min<size_t>((size_t)cap, constraint->table.size()), out);
  return FW_OK;
}

// step graphs the model's decode group has captured (and instantiated) since the model was created, all lanes together
int32_t fw_test_graph_captures(const fw_model* fm, int64_t* out) {
  FW_CHECK_ARG(fm && out, "null argument");
  const Model* m = fm->impl.decoder ? fm->impl.decoder : &fm->impl;
  *out = m->grp.graph_captures.load();
  return FW_OK;
}

// ---------------------------------------------------------------------------------------------------
// Test hooks of the decode-state kernels (tests/test_gpu_decode_state.py).  Each takes its geometry from arguments (not
// from the model) and calls the product's launcher unchanged.  EVERY quantity a kernel turns into an index or an extent
// is checked before anything is allocated or launched: a mistaken test gets FW_EINVAL, never an out-of-bounds access.
// ---------------------------------------------------------------------------------------------------
// ONE launch of dec_beam_update_kernel (fwd::launch_beam_update) for B chunks of K beams at decode step `step`.
// (lp: the log-prob arrays of fw_test_dec_beam_update_lp; without them the kernel gets null pointers and skips those stores)
struct BeamLpArgs { const float* cand_lp; const float* lphist; float* fin_lp; float* lphist2; };
// (alt: fw_test_dec_beam_update_alt.  ptab [B] | null: a RAGGED launch, chunk c with a prompt of ptab[c] tokens; P must be
//  the shortest of them, the run reaches P + budget, kvidx is [R][max(ptab) - 1 + step] and chunk c's rows use the first
//  ptab[c] - 1 + step bytes of theirs.  fin_path [B][FIN_CAP][NT + 1] IN / OUT | null: the kernel gets a null pointer.)
struct BeamAltArgs { const int32_t* ptab; uint8_t* fin_path; };
static int32_t beam_update_hook(fw_model* fm, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                const int32_t* cand_tok, const int32_t* hist, const uint8_t* kvidx, const float* cum,
                                int32_t sentinel_i, float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin,
                                int32_t* fin_tok, int32_t* fin_len, float* fin_score, float* fin_cum, int32_t* hist2,
                                uint8_t* kvidx2, float* cum2, int32_t* cur_tok, const BeamLpArgs* lp,
                                const BeamAltArgs* alt = nullptr) {
  FW_CHECK_ARG(fm && cand_val && cand_tok && cum && done && n_done && n_fin && fin_tok && fin_len && fin_score &&
                   fin_cum && hist2 && kvidx2 && cum2 && cur_tok, "null argument");
  FW_CHECK_ARG(K >= 1 && K <= 16, "need 1 <= K <= 16 (K = %d)", K);
  FW_CHECK_ARG(B >= 1 && B <= 4096, "need 1 <= B <= 4096 (B = %d)", B);
  FW_CHECK_ARG(NT >= 1 && NT <= 4096 && V >= 1, "need 1 <= NT <= 4096 and V >= 1");
  FW_CHECK_ARG(P >= 1 && step >= 0 && step < NT && (int64_t)P - 1 + step < NT,
               "need P >= 1, 0 <= step < NT and P - 1 + step < NT (P = %d, step = %d, NT = %d)", P, step, NT);
  FW_CHECK_ARG(eot >= 0 && eot < V && max_fin >= 1 && budget >= 1 && lp_pow == lp_pow, "bad eot / max_fin / budget / lp_pow");
  const int R = B * K, C = 2 * K;
  const int32_t* ptab = alt ? alt->ptab : nullptr;
  int Pmax = P;
  for (int c = 0; c < B && ptab; ++c) {   // every chunk live at this step: its position below what the run reaches
    FW_CHECK_ARG(ptab[c] >= P && (int64_t)ptab[c] - 1 + step < std::min<int64_t>(NT, (int64_t)P + budget),
                 "ptab[%d] = %d: need P <= ptab[c] and ptab[c] - 1 + step < min(NT, P + budget)", c, ptab[c]);
    Pmax = std::max(Pmax, ptab[c]);
  }
  const int pos = Pmax - 1 + step;   // bytes per kvidx row (ragged: of the longest prompt)
  FW_CHECK_ARG((step == 0 || hist) && (pos == 0 || kvidx), "null history / slot table");
  FW_CHECK_ARG(!lp || (lp->cand_lp && lp->fin_lp && lp->lphist2 && (step == 0 || lp->lphist)), "null log-prob argument");
  for (int i = 0; i < R * C; ++i)
    FW_CHECK_ARG(cand_tok[i] >= 0 && cand_tok[i] < V, "cand_tok[%d] = %d outside [0, %d)", i, cand_tok[i], V);
  for (int64_t i = 0; i < (int64_t)R * pos; ++i) {   // (ragged: the bytes a row uses)
    if (ptab && i % pos >= ptab[i / pos / K] - 1 + step) continue;
    FW_CHECK_ARG(kvidx[i] < K, "kvidx[%lld] = %d is not a beam of %d", (long long)i, (int)kvidx[i], K);
  }
  for (int c = 0; c < B; ++c)
    FW_CHECK_ARG(n_fin[c] >= 0 && n_fin[c] <= FIN_CAP, "n_fin[%d] = %d outside [0, %d]", c, n_fin[c], FIN_CAP);
  GenDev gp;
  memset(&gp, 0, sizeof(gp));
  gp.B = B; gp.K = K; gp.R = R; gp.P = P; gp.budget = budget; gp.max_fin = max_fin; gp.V = V; gp.n_text_ctx = NT;
  gp.lp_pow = lp_pow; gp.eot = eot; gp.kv_div = 1;
  if (ptab) { gp.ragged = 1; gp.reach = P + budget; }
  // both parity halves: the inputs go to half step & 1, everything else holds the caller's sentinel
  const int cur = step & 1;
  const size_t n_state = 2 * (size_t)R * NT;
  std::vector<int> h2(n_state, sentinel_i), ct(R, sentinel_i);
  std::vector<uint8_t> k2(n_state, (uint8_t)sentinel_i);
  std::vector<float> c2(2 * (size_t)R, sentinel_f), cv((size_t)R * 32, -INFINITY);
  std::vector<int> ctk((size_t)R * 32, 0);
  std::vector<float> cl(lp ? (size_t)R * 32 : 0, -INFINITY), l2(lp ? n_state : 0, sentinel_f);
  for (int r = 0; r < R && lp; ++r) {
    for (int q = 0; q < step; ++q) l2[((size_t)cur * R + r) * NT + q] = lp->lphist[(size_t)r * step + q];
    for (int j = 0; j < C; ++j) cl[(size_t)r * 32 + j] = lp->cand_lp[(size_t)r * C + j];
  }
  for (int r = 0; r < R; ++r) {
    for (int q = 0; q < step; ++q) h2[((size_t)cur * R + r) * NT + q] = hist[(size_t)r * step + q];
    const int pos_r = ptab ? ptab[r / K] - 1 + step : pos;
    for (int q = 0; q < pos_r; ++q) k2[((size_t)cur * R + r) * NT + q] = kvidx[(size_t)r * pos + q];
    c2[(size_t)cur * R + r] = cum[r];
    for (int j = 0; j < C; ++j) {   // the kernel's row stride of 32 candidates
      cv[(size_t)r * 32 + j] = cand_val[(size_t)r * C + j];
      ctk[(size_t)r * 32 + j] = cand_tok[(size_t)r * C + j];
    }
  }
  Model* m = &fm->impl;
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  float *d_cv, *d_c2, *d_fs, *d_fc, *d_cl = nullptr, *d_l2 = nullptr, *d_flp = nullptr;
  int *d_ct, *d_h2, *d_cur, *d_step, *d_done, *d_ndone, *d_nfin, *d_ft, *d_fl;
  uint8_t* d_k2;
  const size_t n_f = (size_t)B * FIN_CAP;
  int rc;
  if ((rc = db.upload(&d_cv, cv.data(), cv.size())) || (rc = db.upload(&d_ct, ctk.data(), ctk.size())) ||
      (rc = db.upload(&d_h2, h2.data(), n_state)) || (rc = db.upload(&d_k2, k2.data(), n_state)) ||
      (rc = db.upload(&d_c2, c2.data(), c2.size())) || (rc = db.upload(&d_cur, ct.data(), ct.size())) ||
      (rc = db.upload(&d_step, &step, 1)) || (rc = db.upload(&d_done, done, (size_t)B)) ||
      (rc = db.upload(&d_ndone, n_done, 1)) || (rc = db.upload(&d_nfin, n_fin, (size_t)B)) ||
      (rc = db.upload(&d_ft, fin_tok, n_f * NT)) || (rc = db.upload(&d_fl, fin_len, n_f)) ||
      (rc = db.upload(&d_fs, fin_score, n_f)) || (rc = db.upload(&d_fc, fin_cum, n_f)))
    return rc;
  if (lp && ((rc = db.upload(&d_cl, cl.data(), cl.size())) || (rc = db.upload(&d_l2, l2.data(), n_state)) ||
             (rc = db.upload(&d_flp, lp->fin_lp, n_f * (NT + 1)))))
    return rc;
  int* d_ptab = nullptr;
  uint8_t* d_path = nullptr;
  if (ptab && (rc = db.upload(&d_ptab, ptab, (size_t)B))) return rc;
  if (alt && alt->fin_path && (rc = db.upload(&d_path, (const uint8_t*)alt->fin_path, n_f * (NT + 1)))) return rc;
  fwd::launch_beam_update(nullptr, gp, d_cv, d_ct, d_h2, d_c2, d_k2, d_cur, d_step, d_done, d_ndone, d_nfin, d_ft, d_fl,
                          d_fs, d_fc, d_cl, d_l2, d_flp, d_ptab, d_path);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  if (d_path && (rc = download(alt->fin_path, d_path, n_f * (NT + 1)))) return rc;
  if ((rc = download(hist2, d_h2, n_state)) || (rc = download(kvidx2, d_k2, n_state)) ||
      (rc = download(cum2, d_c2, c2.size())) || (rc = download(cur_tok, d_cur, (size_t)R)) ||
      (rc = download(done, d_done, (size_t)B)) || (rc = download(n_done, d_ndone, 1)) ||
      (rc = download(n_fin, d_nfin, (size_t)B)) || (rc = download(fin_tok, d_ft, n_f * NT)) ||
      (rc = download(fin_len, d_fl, n_f)) || (rc = download(fin_score, d_fs, n_f)) ||
      (rc = download(fin_cum, d_fc, n_f)))
    return rc;
  if (lp && ((rc = download(lp->lphist2, d_l2, n_state)) || (rc = download(lp->fin_lp, d_flp, n_f * (NT + 1))))) return rc;
  return FW_OK;
}

int32_t fw_test_dec_beam_update(fw_model* fm, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                const int32_t* cand_tok, const int32_t* hist, const uint8_t* kvidx, const float* cum,
                                int32_t sentinel_i, float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin,
                                int32_t* fin_tok, int32_t* fin_len, float* fin_score, float* fin_cum, int32_t* hist2,
                                uint8_t* kvidx2, float* cum2, int32_t* cur_tok) {
  return beam_update_hook(fm, B, K, NT, V, P, step, budget, max_fin, lp_pow, eot, cand_val, cand_tok, hist, kvidx, cum,
                          sentinel_i, sentinel_f, done, n_done, n_fin, fin_tok, fin_len, fin_score, fin_cum, hist2, kvidx2,
                          cum2, cur_tok, nullptr);
}

int32_t fw_test_dec_beam_update_lp(fw_model* fm, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                   int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                   const int32_t* cand_tok, const float* cand_lp, const int32_t* hist,
                                   const float* lphist, const uint8_t* kvidx, const float* cum, int32_t sentinel_i,
                                   float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin, int32_t* fin_tok,
                                   int32_t* fin_len, float* fin_score, float* fin_cum, float* fin_lp, int32_t* hist2,
                                   float* lphist2, uint8_t* kvidx2, float* cum2, int32_t* cur_tok) {
  FW_CHECK_ARG(cand_lp && fin_lp && lphist2, "null argument");
  const BeamLpArgs lp{cand_lp, lphist, fin_lp, lphist2};
  return beam_update_hook(fm, B, K, NT, V, P, step, budget, max_fin, lp_pow, eot, cand_val, cand_tok, hist, kvidx, cum,
                          sentinel_i, sentinel_f, done, n_done, n_fin, fin_tok, fin_len, fin_score, fin_cum, hist2, kvidx2,
                          cum2, cur_tok, &lp);
}

int32_t fw_test_dec_beam_update_alt(fw_model* fm, int32_t B, int32_t K, int32_t NT, int32_t V, int32_t P, int32_t step,
                                    int32_t budget, int32_t max_fin, float lp_pow, int32_t eot, const float* cand_val,
                                    const int32_t* cand_tok, const float* cand_lp, const int32_t* hist,
                                    const float* lphist, const uint8_t* kvidx, const float* cum, int32_t sentinel_i,
                                    float sentinel_f, int32_t* done, int32_t* n_done, int32_t* n_fin, int32_t* fin_tok,
                                    int32_t* fin_len, float* fin_score, float* fin_cum, float* fin_lp, int32_t* hist2,
                                    float* lphist2, uint8_t* kvidx2, float* cum2, int32_t* cur_tok, const int32_t* ptab,
                                    uint8_t* fin_path) {
  FW_CHECK_ARG(cand_lp && fin_lp && lphist2, "null argument");
  const BeamLpArgs lp{cand_lp, lphist, fin_lp, lphist2};
  const BeamAltArgs alt{ptab, fin_path};
  return beam_update_hook(fm, B, K, NT, V, P, step, budget, max_fin, lp_pow, eot, cand_val, cand_tok, hist, kvidx, cum,
                          sentinel_i, sentinel_f, done, n_done, n_fin, fin_tok, fin_len, fin_score, fin_cum, hist2, kvidx2,
                          cum2, cur_tok, &lp, &alt);
}

// ONE launch of the alternatives gather (fwd::launch_alt_gather) on caller-provided step-major alt_tok / alt_lp
// [steps][R][n_alt], paths fin_path [R / K][FIN_CAP][NT + 1] and n_hyp hypotheses (chunk, finished slot, length, closing
// step | -1); out_tok / out_lp [n_hyp][T + 1][n_alt] IN / OUT.  Everything the kernel turns into an index is checked first.
int32_t fw_test_alt_gather(fw_model* fm, const int32_t* alt_tok, const float* alt_lp, int32_t steps, int32_t R, int32_t K,
                           int32_t NT, int32_t n_alt, const uint8_t* fin_path, int32_t n_hyp, const int32_t* hyp_chunk,
                           const int32_t* hyp_fin, const int32_t* hyp_len, const int32_t* hyp_end, int32_t T,
                           int32_t* out_tok, float* out_lp) {
  FW_CHECK_ARG(fm && alt_tok && alt_lp && fin_path && hyp_chunk && hyp_fin && hyp_len && hyp_end && out_tok && out_lp,
               "null argument");
  FW_CHECK_ARG(n_alt >= 1 && n_alt <= FW_MAX_ALTERNATIVES, "n_alt %d not in [1, %d]", n_alt, FW_MAX_ALTERNATIVES);
  FW_CHECK_ARG(K >= 1 && K <= 16 && R >= K && R <= 4096 && R % K == 0, "need 1 <= K <= 16, R a multiple of K, R <= 4096");
  FW_CHECK_ARG(NT >= 1 && NT <= 4096 && steps >= 1 && steps <= NT + 1 && T >= 0 && T <= NT && n_hyp >= 1 && n_hyp <= 65535,
               "need 1 <= NT <= 4096, 1 <= steps <= NT + 1, 0 <= T <= NT, 1 <= n_hyp <= 65535");
  const int B = R / K;
  std::vector<fwd::AltHyp> hyps((size_t)n_hyp);
  for (int i = 0; i < n_hyp; ++i) {
    FW_CHECK_ARG(hyp_chunk[i] >= 0 && hyp_chunk[i] < B && hyp_fin[i] >= 0 && hyp_fin[i] < FIN_CAP,
                 "hypothesis %d: chunk %d / finished slot %d out of range", i, hyp_chunk[i], hyp_fin[i]);
    FW_CHECK_ARG(hyp_len[i] >= 0 && hyp_len[i] <= std::min(T, steps) && hyp_end[i] >= -1 && hyp_end[i] < steps,
                 "hypothesis %d: length %d / closing step %d out of range", i, hyp_len[i], hyp_end[i]);
    const uint8_t* path = fin_path + ((size_t)hyp_chunk[i] * FIN_CAP + hyp_fin[i]) * (NT + 1);
    for (int q = 0; q < steps; ++q)
      if (q < hyp_len[i] || q == hyp_end[i])
        FW_CHECK_ARG(path[q] < K, "hypothesis %d: path byte %d = %d is not a beam of %d", i, q, (int)path[q], K);
    hyps[i] = {hyp_chunk[i], hyp_fin[i], hyp_len[i], hyp_end[i]};
  }
  Model* m = &fm->impl;
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  const size_t n_a = (size_t)steps * R * n_alt, n_o = (size_t)n_hyp * (T + 1) * n_alt;
  int *d_at, *d_ot;
  float *d_al, *d_ol;
  uint8_t* d_path;
  fwd::AltHyp* d_h;
  int rc;
  if ((rc = db.upload(&d_at, (const int*)alt_tok, n_a)) || (rc = db.upload(&d_al, alt_lp, n_a)) ||
      (rc = db.upload(&d_path, fin_path, (size_t)B * FIN_CAP * (NT + 1))) || (rc = db.upload(&d_h, hyps.data(), hyps.size())) ||
      (rc = db.upload(&d_ot, (const int*)out_tok, n_o)) || (rc = db.upload(&d_ol, (const float*)out_lp, n_o)))
    return rc;
  fwd::launch_alt_gather(nullptr, d_at, d_al, d_path, d_h, n_hyp, R, K, NT, n_alt, T, d_ot, d_ol);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  if ((rc = download(out_tok, d_ot, n_o))) return rc;
  return download(out_lp, d_ol, n_o);
}

// ONE launch of dec_embed_kernel (fwd::launch_embed): x [rows][d] and the fragment-major copy, un-permuted on the host
// into x_frag [ceil(rows / 16) * 16][d] (the device buffer starts as `sentinel`, so the padding rows of the last 16-row
// tile show whether they were touched).  Position: blk_n > 0: pos_fixed + r % blk_n; else pos_fixed >= 0: pos_fixed;
// else P - 1 + the device step counter (= step).
int32_t fw_test_dec_embed(fw_model* fm, const int32_t* tok, int32_t rows, const float* emb, int32_t V,
                          const float* pos_emb, int32_t NT, int32_t d, int32_t pos_fixed, int32_t P, int32_t step,
                          int32_t blk_n, float sentinel, float* x, float* x_frag) {
  FW_CHECK_ARG(fm && tok && emb && pos_emb && x && x_frag, "null argument");
  FW_CHECK_ARG(rows >= 1 && rows <= 65536 && V >= 1 && NT >= 1 && NT <= 65536, "bad geometry");
  FW_CHECK_ARG(d >= 32 && d % 32 == 0 && d <= 16384, "need d %% 32 == 0, 32 <= d <= 16384 (d = %d)", d);
  FW_CHECK_ARG(blk_n >= 0 && blk_n <= 16, "need 0 <= blk_n <= 16 (blk_n = %d)", blk_n);
  if (blk_n > 0) {
    FW_CHECK_ARG(rows % blk_n == 0, "rows (%d) must be a multiple of blk_n (%d)", rows, blk_n);
    FW_CHECK_ARG(pos_fixed >= 0 && pos_fixed + blk_n <= NT, "positions %d..%d outside [0, %d)", pos_fixed,
                 pos_fixed + blk_n - 1, NT);
  } else if (pos_fixed >= 0) {
    FW_CHECK_ARG(pos_fixed < NT, "position %d outside [0, %d)", pos_fixed, NT);
  } else {
    FW_CHECK_ARG(P >= 1 && step >= 0 && step < NT && (int64_t)P - 1 + step < NT,
                 "need P >= 1, 0 <= step < NT and P - 1 + step < NT (P = %d, step = %d, NT = %d)", P, step, NT);
  }
  for (int r = 0; r < rows; ++r) FW_CHECK_ARG(tok[r] >= 0 && tok[r] < V, "tok[%d] = %d outside [0, %d)", r, tok[r], V);
  const int R16 = (rows + 15) / 16 * 16;
  std::vector<half_t> hx((size_t)rows * d, (half_t)sentinel), hf((size_t)R16 * d, (half_t)sentinel);
  Model* m = &fm->impl;
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  half_t *d_e, *d_p, *d_x, *d_f;
  int *d_tok, *d_step;
  int rc;
  if ((rc = db.upload_f16(&d_e, emb, (size_t)V * d)) || (rc = db.upload_f16(&d_p, pos_emb, (size_t)NT * d)) ||
      (rc = db.upload(&d_x, hx.data(), hx.size())) || (rc = db.upload(&d_f, hf.data(), hf.size())) ||
      (rc = db.upload(&d_tok, tok, (size_t)rows)) || (rc = db.upload(&d_step, &step, 1)))
    return rc;
  fwd::launch_embed(nullptr, d_tok, d_e, d_p, d_x, d_f, rows, d, d_step, pos_fixed, P, blk_n);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  if ((rc = download(hx.data(), d_x, hx.size())) || (rc = download(hf.data(), d_f, hf.size()))) return rc;
  for (size_t i = 0; i < hx.size(); ++i) x[i] = (float)hx[i];
  for (int r = 0; r < R16; ++r)   // fragment-major -> row-major, the padding rows of the last tile included
    for (int k = 0; k < d; ++k) x_frag[(size_t)r * d + k] = (float)hf[frag_pos(r, k, d, 32)];
  return FW_OK;
}

// align_stats_kernel then align_filter_kernel as fw_align launches them (decoder.hip: launch_align_post), on
// caller-provided probabilities probs [B][n_sel][n_tok_cap][T], per-chunk token and frame counts and the median width.  mat
// [B][n_tok_cap][T] is IN / OUT: the device buffer starts as the caller's values, so entries with tok >= n_tok[b] or
// t >= nfr[b] show whether they were touched.  A frame whose probabilities are equal over the tokens has zero variance:
// 1 / sqrt(0) = inf times a zero difference is NaN, in the kernel and in the oracle alike; tests keep the variance
// positive and do not pin that case.
int32_t fw_test_align_post(fw_model* fm, const float* probs, int32_t B, int32_t n_sel, int32_t n_tok_cap, int32_t T,
                           const int32_t* n_tok, const int32_t* nfr, int32_t width, float* mat) {
  FW_CHECK_ARG(fm && probs && n_tok && nfr && mat, "null argument");
  FW_CHECK_ARG(B >= 1 && B <= 65535 && n_sel >= 1 && n_sel <= 65535 && n_tok_cap >= 1 && n_tok_cap <= 65535 && T >= 1 &&
                   T <= (1 << 20), "bad geometry (B, n_sel, n_tok_cap in 1..65535, T >= 1)");
  FW_CHECK_ARG(width >= 1 && width <= 15 && (width & 1), "median_filter_width must be odd and <= 15");
  for (int b = 0; b < B; ++b) {
    FW_CHECK_ARG(n_tok[b] >= 1 && n_tok[b] <= n_tok_cap, "n_tok[%d] = %d outside [1, %d]", b, n_tok[b], n_tok_cap);
    FW_CHECK_ARG(nfr[b] >= 1 && nfr[b] <= T, "nfr[%d] = %d outside [1, %d]", b, nfr[b], T);
  }
  Model* m = &fm->impl;
  FW_HIP(hipSetDevice(m->device));
  HookBufs db;
  const size_t n_probs = (size_t)B * n_sel * n_tok_cap * T, n_stats = (size_t)B * n_sel * T * 2,
               n_mat = (size_t)B * n_tok_cap * T;
  float *d_p, *d_s, *d_m;
  int *d_nt, *d_nf;
  int rc;
  if ((rc = db.upload(&d_p, probs, n_probs)) || (rc = db.alloc(&d_s, n_stats)) ||
      (rc = db.upload(&d_m, mat, n_mat)) || (rc = db.upload(&d_nt, n_tok, (size_t)B)) ||
      (rc = db.upload(&d_nf, nfr, (size_t)B)) || (rc = db.zero(d_s, n_stats * sizeof(float), nullptr)))
    return rc;
  launch_align_post(nullptr, d_p, d_s, n_sel, n_tok_cap, T, B, d_nt, d_nf, width, d_m);
  FW_HIP(hipGetLastError());
  FW_HIP(hipDeviceSynchronize());
  return download(mat, d_m, n_mat);
}

}  // extern "C"
