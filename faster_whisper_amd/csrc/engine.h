// Engine-internal structures of libfwamd.so (host side, C++17).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fwamd.h"
#include "common.h"
#include "kernels.h"

namespace fw {

void set_error(const char* fmt, ...);
#define FW_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      fw::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return FW_ENODEV;                                                                \
    }                                                                                  \
  } while (0)
// FW_HIP inside a helper that several entry points share: a failed call is reported with the caller's own message and
// return code (fw_align: "align setup failed: ..." / FW_ERUNTIME; elsewhere FW_ENODEV, like FW_HIP)
struct HipFail { int code; const char* what; };
#define FW_HIP_AS(f, call)                                                          \
  do {                                                                              \
    hipError_t e_ = (call);                                                         \
    if (e_ != hipSuccess) {                                                         \
      fw::set_error("%s failed: %s", (f).what, hipGetErrorString(e_));             \
      return (f).code;                                                              \
    }                                                                               \
  } while (0)
#define FW_CHECK_ARG(cond, ...)        \
  do {                                 \
    if (!(cond)) {                     \
      fw::set_error(__VA_ARGS__);      \
      return FW_EINVAL;                \
    }                                  \
  } while (0)

// ---- fp16 helpers (host) ----------------------------------------------------------------
inline uint16_t f32_to_f16_bits(float f) {
  half_t h = (half_t)f;  // round-to-nearest-even, same as the device cast
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}
inline float f16_bits_to_f32(uint16_t u) {
  half_t h;
  memcpy(&h, &u, 2);
  return (float)h;
}

// int8_float16 weight row (K25, [CT2-ext] CTranslate2 convention): scale = 127 / absmax(row), q = rint(row * scale)
// (round-half-even).  `row` is K fp16-rounded values; code k goes to q[at(k)] (row-major for the blob and the encoder GEMM,
// fragment-major for the decoder linears); returns the DE-quantisation factor absmax / 127 (1 for an all-zero row).
// The one statement of it: the weight packer and the test hooks that quantise a caller's W both call it.
template <typename At>
inline float quant_row_i8(const float* row, int K, int8_t* q, At&& at) {
  float amax = 0.f;
  for (int k = 0; k < K; ++k) amax = std::max(amax, fabsf(row[k]));
  const float sc = amax > 0.f ? 127.0f / amax : 0.f;
  for (int k = 0; k < K; ++k) q[at(k)] = (int8_t)lrintf(row[k] * sc);
  return amax > 0.f ? amax / 127.0f : 1.0f;
}

// Fragment-major position of element (row, k) of a [rows][K] operand of the decoder linears (dec_kernels.hip): 16-row
// tiles x k-steps of KE elements (fp16: 32, int8: 64); the 16 bytes lane l = 16*((k / (KE/4)) % 4) + row % 16 feeds to the
// MFMA for k-step ks of tile nt sit at ((nt * K/KE + ks) * 64 + l) * 16 B.  The one statement of it: the weight packer
// permutes through it, the test hooks permute and un-permute through it.
inline size_t frag_pos(int64_t row, int64_t k, int64_t K, int KE) {
  const int OCT = KE / 4;
  return (size_t)((((row >> 4) * (K / KE) + k / KE) * 64 + ((k / OCT) & 3) * 16 + (row & 15)) * OCT + (k % OCT));
}

// ---- weight blob (what travels over RCCL at load time) --------------------------------
#define FW_BLOB_MAGIC "FWAMDBL1"
constexpr int kBlobGeneration = 6;   // BlobHeader::reserved (engine.hip: check_blob_header)
struct BlobHeader {
  char magic[8];
  int32_t version;
  int32_t n_tensors;
  int64_t total_bytes;
  int32_t compute_type;
  int32_t reserved;
  fw_config cfg;
};
struct BlobEntry {
  char name[64];
  int32_t dtype;  // 1 = f16, 2 = i8, 0 = f32
  int32_t ndim;
  int64_t dims[4];
  int64_t offset;  // from blob start, 256-byte aligned
  int64_t nbytes;
};

struct LinearW {           // y = x W^T + b ; W [N][K] fp16 (or int8 + per-row scale)
  const half_t* w = nullptr;
  const half_t* b = nullptr;
  const int8_t* wq = nullptr;    // int8 weights [N][K]           (int8_float16 only)
  const float* wscale = nullptr; // dequant scale per output row  (int8_float16 only)
  // LayerNorm-folded form (decoder): w = W.g, y = rstd*(w x - mu*s1) + cf   (engine.hip Packer::folded)
  const float* s1 = nullptr;
  const float* cf = nullptr;
  int N = 0, K = 0;
};
struct LNW { const half_t* g = nullptr; const half_t* b = nullptr; };

struct EncLayerW { LNW ln1, ln2; LinearW qk, v, out, ffn1, ffn2; };
// fp16: qkv, cq, ffn1 are LN-folded; a blob packed with FWAMD_LN_UNFOLD also carries the plain weights (qkv_p, cq_p, ffn1_p) and ln1/2/3 for the
// explicit-LayerNorm evaluation (Model::ln_unfold); int8_float16: explicit LayerNorms feeding the quantiser
struct DecLayerW { LNW ln1, ln2, ln3; LinearW qkv, out, cq, ck, cv, cout, ffn1, ffn2; LinearW qkv_p, cq_p, ffn1_p; };

enum ProfFamily {
  PF_LOGMEL = 0, PF_ENC_GEMM, PF_ENC_ATTN, PF_ENC_LN, PF_CROSS_KV_GEMM,
  PF_DEC_GEMM_QKV, PF_DEC_GEMM_DXD, PF_DEC_GEMM_FFN1, PF_DEC_GEMM_FFN2,
  PF_DEC_SELF_ATTN, PF_DEC_CROSS_ATTN, PF_DEC_LOGITS, PF_DEC_SAMPLE, PF_DEC_MISC, PF_COUNT
};

struct ProfAcc {
  double ms = 0; int64_t launches = 0; double flops = 0; double bytes = 0;
};

// One profiling recorder, for the scopes of ONE stream: the model has one for its encoder stream, every decode lane one
// for its own.  The mutex is there for the readers (fw_prof_get / fw_prof_reset, any thread).
struct Prof {
  std::mutex mu;
  bool on = false;
  ProfAcc acc[PF_COUNT];
  struct PendingEv { hipEvent_t a, b; int fam; };
  std::vector<PendingEv> pending;
  std::vector<hipEvent_t> ev_pool;
  ~Prof();
};

int dev_alloc(void** p, size_t bytes);
template <typename T>
inline int dev_alloc_t(T** p, size_t n) { return dev_alloc(reinterpret_cast<void**>(p), n * sizeof(T)); }
// Device buffers of one owner (a Model, a GenWorkspace, one fw_align call, one test-hook call): a buffer is recorded
// where it is allocated, and all of them are freed with the owner, however the owner goes.
struct DevBufs {
  std::vector<void*> ptrs;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  int alloc(T** p, size_t n) {
    if (int rc = dev_alloc_t(p, n)) return rc;
    ptrs.push_back(*p);
    return FW_OK;
  }
  template <typename T>
  int zalloc(T** p, size_t n) {   // ... and zeroed (on the null stream: the owner synchronises before its first use)
    if (int rc = alloc(p, n)) return rc;
    FW_HIP(hipMemset(*p, 0, n * sizeof(T)));
    return FW_OK;
  }
};
// A device buffer that grows by replacement (the old contents go), freed with its owner.
template <typename T>
struct GrowBuf {
  T* p = nullptr;
  int64_t cap = 0;   // elements
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { if (p) (void)hipFree(p); }
  int ensure(int64_t n) {
    if (n <= cap) return FW_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (int rc = dev_alloc_t(&p, (size_t)n)) return rc;
    cap = n;
    return FW_OK;
  }
};

// int8_float16: the quantised input rows of the encoder GEMM — codes [rows][ld] and per-row de-quantisation scales [rows].
// The capacity is set where the two buffers are allocated; quantise_rows (below) fills them and records what they hold.
struct QuantRows {
  int8_t* q = nullptr;
  float* scale = nullptr;
  int64_t cap_rows = 0, cap_elems = 0;
  int64_t rows = 0, ld = 0;   // held now
  bool fits(int64_t r, int64_t K) const { return r >= 0 && K >= 0 && r <= cap_rows && r * K <= cap_elems; }
};

struct Model;
// Encoder-output buffers of one model, every one [max_batch][T][d] halves (hipMalloc / hipFree synchronise the whole
// device and would serialise the replicas that share a GPU).  The model and each of its tensors hold the pool: a tensor
// gives its buffer back to the pool it was taken from, whenever it is freed — after fw_model_free (which closes the
// pool) the buffer is released instead.  A buffer can therefore never reach a pool of another size.
struct EncPool {
  std::mutex mu;
  std::vector<half_t*> free;
  const size_t elems;               // of every buffer
  bool closed = false;
  std::atomic<Model*> model;        // null once closed (decoder.hip asks which decode group a tensor belongs to)
  EncPool(Model* m, size_t elems_) : elems(elems_), model(m) {}
  int take(half_t** p);             // engine.hip
  void give(half_t* p);
  void close();
};
struct Tensor {  // fw_tensor
  std::shared_ptr<EncPool> pool;
  half_t* data = nullptr;  // [B][T][D] fp16, device
  int B = 0, T = 0, D = 0;
  uint64_t id = 0;         // unique per encoder output (cross-K/V cache key)
};

struct GenWorkspace;  // decoder-side buffers of one decode lane (decoder.hip)
struct GenRequest;    // one fw_generate call waiting to be decoded (decoder.hip)
struct CrossPool;     // cross-attention K / V^T of the encoder outputs in flight, shared by the lanes (decoder.hip)

// Decode LANE of a decode group: a decode workspace, the stream its runs are launched on (and `spare`); n lanes: n runs
// in flight, the HBM-bound cross-attention of one beside the linears of the other: two lanes +8 % (profiles/
// r03_two_groups_probe.txt; 3 / 4 lanes: r06_ab_lanes.jsonl).  Config, weights, pool and sizes are the model's.
constexpr int kMaxDecodeLanes = 4;
struct DecodeLane {
  GenWorkspace* gen = nullptr;    // created on first use, or by fw_model_set_decode_batch (decoder.hip)
  hipStream_t stream = nullptr;   // created with the workspace (role "DEC") and kept until the lane goes
  hipStream_t spare = nullptr;    // lanes 1 ..: IDLE second stream; four lanes are 4.5 % slower without
  std::mutex mu;                  // held by whoever runs on the lane: a decode run, fw_detect_language, fw_align
  Prof prof;                      // the decode scopes recorded on `stream`
  bool busy = false;              // a run of the group has taken the lane (under DecodeGroup::mu)
  ~DecodeLane();                  // waits for the stream, then frees the workspace and the streams (decoder.hip)
};

// Decode group of a device: the worker replicas that share one decode workspace.  Concurrent fw_generate calls
// whose options agree (decoder.hip: mergeable(); the prompt length need not) are merged into ONE decode run (their rows
// share every weight byte streamed per step);
// the first caller that finds no run in progress leads it, the others wait for their results.
struct DecodeGroup {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<GenRequest*> queue;
  bool gathering = false;         // a caller is collecting the requests of the next run (one at a time)
  bool resizing = false;          // fw_model_set_decode_batch is rebuilding the workspaces / the lanes: callers wait
  int active_runs = 0;            // runs in flight (<= lanes of the group)
  std::atomic<int> lanes_enabled{kMaxDecodeLanes};   // fw_model_set_decode_lanes: runs allowed in flight
  std::atomic<int> encoding{0};   // member encodes in flight: requests that are about to arrive
  std::chrono::steady_clock::time_point last_arrival{};   // when the newest request was queued
  std::mutex enc_mu;              // one encoder pass at a time per device
  std::atomic<int> enc_pass_us{0};   // running mean of the time a member holds enc_mu (one encoder pass)
  std::atomic<int> merge_wait_ms{-1};   // fw_model_set_merge_wait: -1 = 2.5 encoder passes (<= 250 ms), 0 = never wait
  std::atomic<int> merge_fill_pct{90};  // ... and the share of a run's chunk capacity at which the leader stops waiting
  // statistics (fw_model_decode_stats): decode runs, fw_generate calls served, chunks decoded, largest run
  std::atomic<int64_t> n_runs{0}, n_requests{0}, n_chunks{0};
  std::atomic<int> max_run_chunks{0};
  std::atomic<int64_t> graph_captures{0};   // step graphs captured and instantiated by the group's lanes (fw_test_graph_captures)
};

// Where the kernels find the weights inside a blob: filled by the one walk over the weight list (engine.hip:
// walk_weights), which the packer and the binder both make.
struct Weights {
  int c_pad = 0;  // mel channels padded to a multiple of 64 for the conv1 GEMM
  LinearW conv1, conv2;
  const half_t* enc_pos = nullptr;
  std::vector<EncLayerW> enc;
  LNW enc_ln_post;
  const half_t* tok_emb = nullptr;  // [V][d]
  const half_t* dec_pos = nullptr;  // [n_text_ctx][d]
  std::vector<DecLayerW> dec;
  LinearW logits;  // final LN folded into the tied-embedding projection (fp16) / int8 tied embedding
  LinearW logits_p;   // fp16: the tied embedding itself, fragment-major (explicit final LayerNorm, ln_unfold >= 1)
  LNW dec_ln;
};
// host only: the header is one this library packs for a blob of blob_bytes bytes; then every tensor the walk expects for
// the header's config and compute type is in `entries` with the dtype, dims, size, alignment and bounds the walk implies
// (FW_EINVAL with the tensor's name otherwise), and W points into `blob`.  *has_plain: the explicit-LayerNorm forms travel.
int check_blob_header(const BlobHeader& h, int64_t blob_bytes);
int bind_weights(const BlobHeader& h, const BlobEntry* entries, void* blob, Weights& W, bool* has_plain);

struct Model : Weights {
  fw_config cfg{};
  int compute_type = 0;
  int device = 0;
  int max_batch = 0, max_beam = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;

  void* blob = nullptr;     // device blob (owned unless external)
  bool blob_owned = true;
  int64_t blob_bytes = 0;
  // fp16 evaluation order of the decoder LayerNorms.  0: folded into the consuming linear (one
  // launch fewer per LayerNorm; W o g is rounded to fp16 once more and the normalised row is never rounded); 1: the final
  // LayerNorm is its own kernel — fp16(LN(x)) times the tied embedding, the rounding points of the reference's fp16
  // path; 2: every decoder LayerNorm is.  FWAMD_LN_UNFOLD in the environment when the blob is PACKED (the plain weight
  // forms then travel in it: has_plain) and when the model is created.  A diagnostic; default off.
  int ln_unfold = 0;
  bool has_plain = false;

  // log-mel constants
  float* lm_consts = nullptr;  // cos table [400] + hann [400]
  float* lm_filtT = nullptr;   // [224][mel_pad]
  int lm_mel_pad = 0;

  // encoder workspaces (sized for max_batch), the log-mel constants among them, all owned by `bufs`
  DevBufs bufs;
  GrowBuf<float> ws_pcm;
  int64_t* ws_offsets = nullptr;
  GrowBuf<float> ws_raw;                              // raw log-mel [B][n_mels][stride]
  int* ws_chunk_max = nullptr;
  int* ws_nframes = nullptr;
  float* ws_feat32 = nullptr;                         // [B][n_mels][3000]
  half_t* ws_mel_cl = nullptr;                        // [B][3002][c_pad]
  half_t* ws_conv1 = nullptr;                         // [B][3002][d]
  half_t *ws_x = nullptr, *ws_x2 = nullptr, *ws_xn = nullptr;  // [B][1500][d]
  half_t* ws_qk = nullptr;                            // [B][1500][2d]
  half_t* ws_vt = nullptr;                            // [B][d][t_pad]
  half_t* ws_att = nullptr;                           // [B][1500][d]
  half_t* ws_ffn = nullptr;                           // [B][1500][4d]
  QuantRows ws_xq;                                    // int8_float16: quantised GEMM input, up to [B*1500][4d]
  int t_pad = 0;

  // decode side.  A model either owns a decode group (lanes[0] from model creation, its workspace built on first use
  // for decode_batch chunks; fw_model_set_decode_batch adds lanes) or has joined another model's (decoder != null).
  // Only that rebuild changes the vector: fw_generate waits for it, fw_prof_* and fw_synchronize must not run beside.
  std::vector<std::unique_ptr<DecodeLane>> lanes;
  Model* decoder = nullptr;
  // The cross-attention K / V^T cache is ONE pool per decode group: blocks of max_batch chunk slots, one block per
  // encoder output in flight, handed to whichever lane decodes the request — so every lane can run full-size runs
  // without holding a cache of its own.
  CrossPool* xpool = nullptr;
  int decode_batch = 0;          // chunk slots of the pool (= encoder chunks the group keeps in flight)
  int lane_batch = 0;            // chunks ONE decode run (one lane's workspace) holds; 0: decode_batch
  int decode_self_ctx = 0;   // self-attention cache positions per row at full row capacity (0 = the text context)
  int dependents = 0;        // live models that use this one's weight blob or decode workspace (g_models_mu)
  bool free_deferred = false;   // fw_model_free was called while dependents > 0: freed with the last dependent
  void* self = nullptr;         // the fw_model this Model lives in
  Model* blob_owner = nullptr;  // the model whose blob this one borrows (fw_model_create_from_blob_dev on fw_model_blob)
  DecodeGroup grp;

  std::shared_ptr<EncPool> enc_pool;   // pooled encoder-output buffers, shared with the tensors

  Prof prof;   // the encoder's scopes (recorded on `stream` under mu); the decode scopes are the lanes'
};

// profiling scope: brackets a group of launches with HIP events on st, the stream p's owner launches on
struct ProfScope {
  Prof* p; int fam; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
  ProfScope(Prof& p_, int fam_, double flops, double bytes, hipStream_t st_);
  ProfScope(Model* m, int fam_, double flops, double bytes) : ProfScope(m->prof, fam_, flops, bytes, m->stream) {}
  ~ProfScope();
};
void prof_collect(Prof& p);   // waits for the scopes recorded so far and adds their times

// a non-blocking stream at the priority the environment variable `env` names ("high" / "low"; anything else, or unset:
// the default priority).  ROCm gives every priority level its own hardware queues, so a decode stream created "high"
// neither shares a hardware queue with the encoder streams of the workers nor waits behind their workgroups when a CU
// frees up.  Measurement knob: FWAMD_DEC_STREAM_PRIO (decode lanes), FWAMD_ENC_STREAM_PRIO (encoder / replica streams).
hipError_t create_stream(hipStream_t* st, const char* role);   // role "ENC" / "DEC": engine.hip
// decode groups (decoder.hip): chunks an idle two-lane group waits for before it leads a run
int64_t idle_lead_chunks(int64_t queued, int n_queued, int encoding, int64_t want, int max_batch, int lanes = 2);
// ... and what a lane holds of runs led by one call (decoder.hip; host arithmetic only: fw_test_run_capacity)
struct RunCapacity {
  int64_t rows_per_chunk;        // decoder rows per encoder chunk: beam_size, or num_hypotheses when sampling
  int64_t rows, row_cap, self_cap;   // the leading call's rows; the lane's rows and self-attention row-positions
  int ctx;                       // cache positions per row of the run
  bool rows_fit, cache_fits;     // the leading call alone fits the lane (fw_generate refuses one that does not)
  int64_t want;                  // chunks the leader waits for; 0: it does not wait (sampling)
  int64_t run_cap;               // chunks the run is filled to (take_mergeable)
  RunCapacity(int lane_chunks, int max_batch, int max_beam, int64_t self_cap, int B, bool sampling, int beam_size,
              int num_hypotheses, int ctx);
};

// One launch of the encoder GEMM, a linear layer on "many rows": C = act(A W^T + b) + res (encoder, cross-K/V
// projections).  Strides in elements; what a call site does not name is absent.
struct LinIn {
  const half_t* A = nullptr; int64_t lda = 0, a_bs = 0;     // fp16 input: row m of chunk z at A + z * a_bs + m * lda
  const QuantRows* xq = nullptr;                            // ... or (int8_float16) the [batch * M] rows quantise_rows left
};
struct LinCall {
  LinIn in;
  half_t* C = nullptr; int64_t ldc = 0, c_bs = 0;           // trans: C^T, ldc its row stride
  const half_t* res = nullptr; int64_t ldr = 0, r_bs = 0;   // added after act (r_bs = 0: one block shared by the chunks)
  int M = 0, batch = 1;
  int act = 0;                                              // 1: exact GELU
  bool trans = false;
  int head_rows = 0;                                        // > 0: fragment-major cross-attention K / V^T (kernels.h)
  // n_layers > 1 (fp16): ONE launch for the same linear of consecutive layers on one input — layer l uses L.w + l * w_ls,
  // L.b + l * b_ls and writes C + l * c_ls; gemm.hip "LAYERED launch"
  int n_layers = 1; int64_t w_ls = 0, b_ls = 0, c_ls = 0;
  hipStream_t st = nullptr;                                 // null: the model's encoder stream
};
// the one place that fills the GEMM's parameters; ldw: row stride of the weights (the product's are dense: L.K)
fwk::GemmParams gemm_params(const LinearW& L, const LinCall& c, int64_t ldw);
int run_linear(Model* m, const LinearW& L, const LinCall& c);
// int8_float16 input of a linear (K25): per-row dynamic quantisation of A [rows][K] (dense), through the LayerNorm that
// feeds it when ln is given, into qr — which any number of run_linear calls then read (the fused Q|K and V projections
// share their input, the cross-K/V projections of all layers theirs).  FW_EINVAL when qr cannot hold the rows.
int quantise_rows(Model* m, const half_t* A, const LNW* ln, int64_t rows, int K, hipStream_t st, QuantRows& qr);
void set_cross_kv_layered(int on);                 // decoder.hip: knob 6
// encoder forward on the channel-last mel image already in m->ws_mel_cl; result into out [B][1500][d]
int run_encoder(Model* m, int B, half_t* out);

// decoder entry points (decoder.hip)
void set_pos_blocks(int on);                  // fw_test_knob(4, ..): position blocks for the prompt forward and align
uint64_t next_tensor_id();
int gen_workspace_ensure(Model* dm, DecodeLane* lane);   // built on first use (caller holds lane->mu)
int cross_pool_ensure(Model* dm, int pool_chunks);   // the two steps at explicit sizes (fw_model_set_decode_batch)
int gen_workspace_build(const Model* dm, DecodeLane* lane, int lane_chunks, int self_ctx);
void gen_workspace_free(DecodeLane* lane);
// HBM of one lane's workspace for runs of up to lane_chunks chunks (self_ctx 0 = the text context) — without the
// cross-attention pool, which is cross_pool_bytes(m, pool_chunks) once per group
int64_t gen_workspace_bytes(const Model* m, int lane_chunks, int self_ctx);
int64_t cross_pool_bytes(const Model* m, int pool_chunks);
void cross_pool_free(Model* m);
// align's device post-processing on stream st: align_stats_kernel (standardise over tokens) then align_filter_kernel
// (median over frames, mean over the n_sel heads) on probs [B][n_sel][n_tok_cap][T] -> mat [B][n_tok_cap][T]; stats is
// scratch of [B][n_sel][T][2] floats.  fw_align and its test hook launch the pair through here.
void launch_align_post(hipStream_t st, const float* probs, float* stats, int n_sel, int n_tok_cap, int T, int B,
                       const int* n_tok, const int* nfr, int width, float* mat);
inline Model* decoder_of(Model* m) { return m->decoder ? m->decoder : m; }
inline const Model* decoder_of(const Model* m) { return m->decoder ? m->decoder : m; }
// the decode group an encoder output belongs to; null once the model that made it is gone
inline Model* decoder_of(const Tensor& t) {
  Model* m = t.pool ? t.pool->model.load() : nullptr;
  return m ? decoder_of(m) : nullptr;
}
inline int lane_chunks_of(const Model* m) {
  const int b = m->lane_batch > 0 ? m->lane_batch : m->decode_batch;
  return b > m->max_batch ? b : m->max_batch;
}

}  // namespace fw

struct fw_model { fw::Model impl; };
struct fw_tensor { fw::Tensor impl; };
