// Decoder side of libfwamd.so: cross-K/V projection, KV-cached decode loop with on-device
// logits rules + beam search (hipGraph-replayed step), language detection and
// cross-attention alignment.
//
// Reference interfaces replaced (faster_whisper/transcribe.py):
//   ctranslate2.models.Whisper.generate         :222-236, :1446-1459
//   ctranslate2.models.Whisper.detect_language  :215, :1193, :1823
//   ctranslate2.models.Whisper.align            :1709-1715
// The decoding rules restate CTranslate2 4.x / openai-whisper behaviour (SURVEY.md
// Appendix A); oracle/whisper.py is the CPU statement of the same rules.
//
// Decode groups.  A decode step is HBM-bound: it streams every decoder weight once (1.47 GB for large-v3)
// whatever the number of rows.  CTranslate2 runs `inter_threads` replicas side by side, each streaming the weights
// for its own batch; here the worker replicas of a device share ONE decode workspace sized for all of their
// batches (288 GB of HBM make that cheap), and fw_generate calls that arrive while a run is in progress are
// merged into the next run: up to decode_batch chunks x beam rows share each weight byte and each launch.  The
// encoders of the other workers overlap with the running decode on their own streams (MFMA-bound next to
// HBM-bound).  Results are independent of the merge: every kernel works per row / per chunk.
#include "engine.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <numeric>

#include "dec_kernels.h"
#include "kernels.h"

namespace fw {

using fwd::FIN_CAP;
using fwd::GenDev;

// rows of a merged decode run above which a second, nearly empty round of workgroups starts (dec_kernels.hip)
#define DEC_RUN_MAX_ROWS 1600

// Cross-attention K / V^T pool of a decode group: n_blocks blocks of EB (= max_batch) chunk slots, layer-major
// [L][n_blocks * EB][H][kvp * 64] (a layer's launch sees every slot of that layer behind one base pointer; a run reaches
// its chunks through a slot table).  A block holds the projected K / V^T of ONE encoder output; fw_generate /
// fw_detect_language / fw_align take the block that already holds their encoder output (a hit: generate after
// detect_language, align after generate, the temperature ladder re-decoding a window) or the least recently used free
// one.  A decode run takes all its blocks at once (no hold-and-wait between the lanes).
struct CrossPool {
  DevBufs bufs;                          // ck and cvt, freed with the pool
  half_t *ck = nullptr, *cvt = nullptr;
  int n_blocks = 0, EB = 0, kvp = 0;
  struct Block { uint64_t enc_id = 0; int n = 0; bool busy = false; uint64_t stamp = 0; };
  std::vector<Block> blocks;
  std::mutex mu;
  std::condition_variable cv;
  uint64_t clock = 0;
  int n_slots() const { return n_blocks * EB; }
};

struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  GenDev key;
  uint64_t stamp = 0;
  int forms = 0;    // fwd::kernel_forms_epoch() at capture: a measurement knob that changes which kernels a step
                    // launches (fw_test_knob) must not be answered with a graph captured before it was set
};
// step graphs a workspace keeps (merged runs come in every multiple of a batch up to the lane's capacity: 20 sizes with the
// bench's workers; a cache of 12 re-captured and re-instantiated 261-node graphs all the time)
constexpr size_t kStepGraphSlots = 40;

struct GenWorkspace {
  DevBufs bufs;                          // every device pointer below (gen_workspace_build), freed with the workspace
  int B = 0, K = 0, R = 0, NT = 0;       // capacity of a run: chunks, beams per chunk, rows = B * K
  int EB = 0;                            // chunks of one encoder output (the models' max_batch)
  int* slot_map = nullptr;               // [R] chunk of the run -> chunk slot of the cross-attention pool (device)
  // self-attention cache: ONE allocation of L x self_cap x d halves per K and V, self_cap = R x NTs row-positions.
  // Its geometry is the RUN's: [L][rows of the run][H][ctx of the run][64] with rows x ctx <= self_cap, so a run
  // whose calls ask for max_length 104 holds 4.3x the rows of one that asks for the whole text context.
  half_t *sk = nullptr, *sv = nullptr;
  int NTs = 0;                           // positions per row at full row capacity
  int64_t self_cap = 0;                  // rows x positions
  half_t *x = nullptr, *qkv = nullptr, *att = nullptr, *qc = nullptr, *ffn = nullptr;
  float* logits = nullptr;               // [R][V]
  int* prompt_dev = nullptr;             // [NT][max(R, B)]
  int* prompt_blk = nullptr;             // the same tokens in position-block order: [block][chunk][position of the block]
  int* cur_tok = nullptr;                // [R]
  int* hist2 = nullptr;                  // [2][R][NT]
  float* cum2 = nullptr;                 // [2][R]
  uint8_t* kvidx2 = nullptr;             // [2][R][NT]
  float* cand_val = nullptr;             // [R][32]
  int* cand_tok = nullptr;
  // per-token log-probs, recorded by every run beside their token twins (dec_kernels.h)
  float* cand_lp = nullptr;              // [R][32]
  float* lphist2 = nullptr;              // [2][R][NT]
  float* fin_lp = nullptr;               // [R][FIN_CAP][NT + 1]
  // alternatives (fw_generate_alt; dec_kernels.h): nothing until a run records some (run_alt_ensure), then sized by the largest
  // run so far.  A step graph holds these pointers by value: growing them drops the graphs that record alternatives.
  GrowBuf<int> alt_tok;                  // [steps][rows of the run][n_alt of the run]
  GrowBuf<float> alt_lp;
  GrowBuf<uint8_t> fin_path;             // [R][FIN_CAP][NT + 1]
  GrowBuf<int> alt_out_tok;              // the gather's output: [returned hypotheses][budget + 1][n_alt]
  GrowBuf<float> alt_out_lp;
  GrowBuf<fwd::AltHyp> alt_hyps;
  // phrase boosting (fw_generate_boost): the run's compiled table.  Nothing until the first boosted run, which allocates it
  // at its maximum size (fwd::BOOST_TABLE_MAX_WORDS): the pointer never changes afterwards, so a cached step graph stays
  // valid whatever list the next run brings — the sizes travel in the table's header — and no graph holds a caller's pointer.
  GrowBuf<int> boost_tab;
  // constrained decoding (fw_generate_constrain): the run's compiled table, held the same way (allocated once, by the first
  // constrained run, at fwd::CONSTRAIN_TABLE_MAX_WORDS)
  GrowBuf<int> constrain_tab;
  int *done = nullptr, *n_done = nullptr, *n_fin = nullptr, *fin_tok = nullptr, *fin_len = nullptr;
  float *fin_score = nullptr, *fin_cum = nullptr;
  int* d_step = nullptr;
  float* no_speech = nullptr;
  unsigned long long* sup_bits = nullptr;   // suppress list, one bit per token id
  int* zero_done = nullptr;              // [R] zeros (kernels that take a `done` pointer outside generate)
  // ragged runs (calls of different prompt lengths in one run): prompt length and <sot> position per chunk, and the final
  // hidden rows at the <sot> positions, gathered pass by pass for ONE vocabulary projection (row-major + fragment-major)
  // (per DECODE chunk: a sampling run has num_hypotheses decode chunks per encoder chunk, up to R of them)
  int *ptab = nullptr, *sot_tab = nullptr;   // [R]
  half_t *nsp_x = nullptr, *nsp_xf = nullptr;   // [R rounded up to 16][d]
  // sampling runs: temperature, seed and first row of its call for every decode row (dec_kernels.h)
  fwd::SmpRow* smp_tab = nullptr;            // [R]
  // ... and, for the runs that truncate their draw (fw_generate_trunc), the (top_k, top_p) of every decode row's call
  fwd::TruncRow* trunc_tab = nullptr;        // [R]
  half_t *x_frag = nullptr, *att_frag = nullptr, *ffn_frag = nullptr;   // fragment-major GEMM inputs (fp16)
  half_t* xn_frag = nullptr;             // fp16(LayerNorm(x)), fragment-major (explicit-LayerNorm order, Model::ln_unfold)
  int8_t* xq = nullptr;                  // int8_float16: quantised linear input, fragment-major [R16][4d]
  float* xs = nullptr;                   //               per-row de-quantisation scale [R]
  QuantRows ekq;                         // int8_float16: one encoder output quantised for the cross-K/V projection
  // hipGraphs of the decode step, one per distinct GenDev (merged runs differ in their chunk count)
  std::vector<GraphSlot> graphs;
  uint64_t graph_clock = 0;
  bool graphs_enabled = true;
  ~GenWorkspace() {
    for (GraphSlot& s : graphs)
      if (s.exec) (void)hipGraphExecDestroy(s.exec);
  }
};

static std::atomic<uint64_t> g_tensor_id{1};
uint64_t next_tensor_id() { return g_tensor_id.fetch_add(1); }

// A process-wide on / off knob, on by default: -1 = not read yet — the environment variable `env` is read once, on first
// use (set to 0: off) — otherwise what its setter (fw_test_knob) stored.
static bool env_knob_on(std::atomic<int>& v, const char* env) {
  int x = v.load(std::memory_order_relaxed);
  if (x < 0) {
    const char* e = getenv(env);
    x = (e && atoi(e) == 0) ? 0 : 1;
    v.store(x);
  }
  return x != 0;
}

// positions per cache row at full row capacity: the whole text context when one encoder batch is all the workspace
// holds, otherwise what set_decode_batch chose (>= the share that lets ONE full-context encoder batch run)
static int self_positions(const Model* m, int decode_batch, int nts) {
  const int NT = m->cfg.n_text_ctx;
  const int need = (int)(((int64_t)NT * m->max_batch + decode_batch - 1) / decode_batch);   // EB*K*NT <= B*K*NTs
  return std::min(NT, std::max(std::max(nts, need), 8));
}

int64_t gen_workspace_bytes(const Model* m, int lane_chunks, int nts) {
  const fw_config& c = m->cfg;
  const int64_t B = lane_chunks, R = B * m->max_beam, d = c.d_model, L = c.n_dec_layers, NT = c.n_text_ctx;
  const int64_t NTs = self_positions(m, lane_chunks, nts > 0 ? nts : (int)NT);
  int64_t n = 2 * (L * R * NTs * d) * 2;                               // self K/V (fp16)
  n += R * (int64_t)c.n_vocab * 4 + R * 12 * d * 2 * 2;                // logits, activations
  n += R * FIN_CAP * NT * 4 + 3 * R * NT * 4;                          // finished hypotheses, histories
  n += R * FIN_CAP * (NT + 1) * 4 + 2 * R * NT * 4 + R * 32 * 4;       // their per-token log-probs
  return n + (64 << 20);
}

int64_t cross_pool_bytes(const Model* m, int pool_chunks) {
  const fw_config& c = m->cfg;
  const int64_t kvp = ((c.n_audio_ctx + 31) / 32) * 32;
  return 2 * ((int64_t)c.n_dec_layers * pool_chunks * c.d_model * kvp) * 2;   // K and V^T, fp16
}

// blocks of a pool of `pool_chunks` chunk slots — and, one block per call, the calls a decode run may take
static int pool_block_count(int pool_chunks, int max_batch) {
  return std::max(1, std::max(pool_chunks, max_batch) / max_batch);
}

int cross_pool_ensure(Model* m, int pool_chunks) {
  if (m->xpool) return FW_OK;
  const fw_config& c = m->cfg;
  std::unique_ptr<CrossPool> p(new CrossPool());   // (goes again, with its buffers, unless it is installed below)
  p->EB = m->max_batch;
  p->n_blocks = pool_block_count(pool_chunks, m->max_batch);
  p->kvp = ((c.n_audio_ctx + 31) / 32) * 32;
  p->blocks.assign(p->n_blocks, CrossPool::Block());
  const size_t n = (size_t)c.n_dec_layers * p->n_slots() * c.d_model * p->kvp;
  int rc;
  if ((rc = p->bufs.alloc(&p->ck, n)) || (rc = p->bufs.alloc(&p->cvt, n))) return rc;
  // the padded keys (>= T) are never written: K garbage is masked, V^T must be 0 (0 * NaN)
  const HipFail fail{FW_ENODEV, "cross-attention pool setup"};
  FW_HIP_AS(fail, hipMemset(p->ck, 0, n * sizeof(half_t)));
  FW_HIP_AS(fail, hipMemset(p->cvt, 0, n * sizeof(half_t)));
  FW_HIP_AS(fail, hipDeviceSynchronize());
  m->xpool = p.release();
  return FW_OK;
}

void cross_pool_free(Model* m) {
  delete m->xpool;   // (its DevBufs frees K and V^T)
  m->xpool = nullptr;
}

// Blocks for the encoder outputs `ids` (chunk counts `ns`), ALL of them or none: waits until enough blocks are free.
// blk[i] = block index, hit[i] = the block already holds that encoder output's K / V^T.
static void pool_acquire(CrossPool* p, const std::vector<uint64_t>& ids, const std::vector<int>& ns, std::vector<int>& blk,
                         std::vector<char>& hit) {
  std::unique_lock<std::mutex> lk(p->mu);
  const int n = (int)ids.size();
  blk.assign(n, -1);
  hit.assign(n, 0);
  for (;;) {
    int n_free = 0;
    for (const CrossPool::Block& b : p->blocks) n_free += b.busy ? 0 : 1;
    if (n_free >= n) break;
    p->cv.wait(lk);
  }
  for (int i = 0; i < n; ++i)          // first the hits ...
    for (int k = 0; k < p->n_blocks; ++k) {
      CrossPool::Block& b = p->blocks[k];
      if (!b.busy && b.enc_id == ids[i] && b.n == ns[i] && ids[i] != 0) { b.busy = true; blk[i] = k; hit[i] = 1; break; }
    }
  for (int i = 0; i < n; ++i) {        // ... then the least recently used free blocks
    if (blk[i] >= 0) continue;
    int best = -1;
    for (int k = 0; k < p->n_blocks; ++k)
      if (!p->blocks[k].busy && (best < 0 || p->blocks[k].stamp < p->blocks[best].stamp)) best = k;
    CrossPool::Block& b = p->blocks[best];
    b.busy = true; b.enc_id = 0; b.n = 0;   // marked empty until the projection has been launched
    blk[i] = best;
  }
  for (int i = 0; i < n; ++i) p->blocks[blk[i]].stamp = ++p->clock;
}

static void pool_release(CrossPool* p, const std::vector<int>& blk) {
  {
    std::lock_guard<std::mutex> lk(p->mu);
    for (int k : blk)
      if (k >= 0) p->blocks[k].busy = false;
  }
  p->cv.notify_all();
}

struct PoolHold {   // releases its blocks when the decode run / detect_language / align call ends, however it ends
  CrossPool* p;
  std::vector<int> blk;
  hipStream_t st = nullptr;   // the stream the blocks' projections / readers were launched on
  // A block carries its encoder output's id from the moment the projection is LAUNCHED; the other lane (another stream)
  // may take it as a hit, or recycle it, as soon as it is released.  Every normal return path has synchronised the stream
  // already (this wait then costs nothing); an error return taken earlier must not free blocks that kernels of this
  // stream may still be writing.
  ~PoolHold() {
    if (!p) return;
    if (st && !blk.empty()) (void)hipStreamSynchronize(st);
    pool_release(p, blk);
  }
};

// A workspace is installed whole or not at all: after a failed build (argument check, out of HBM) `ws` goes again with
// what it has allocated, and the next call starts from scratch instead of launching kernels on a half-allocated one.
int gen_workspace_build(const Model* m, DecodeLane* lane, int lane_chunks, int self_ctx) {
  const fw_config& c = m->cfg;
  std::unique_ptr<GenWorkspace> ws(new GenWorkspace());
  GenWorkspace* g = ws.get();
  g->B = lane_chunks;
  g->EB = m->max_batch;
  g->K = m->max_beam;
  g->R = g->B * g->K;
  g->NT = c.n_text_ctx;
  g->NTs = self_positions(m, g->B, self_ctx > 0 ? self_ctx : c.n_text_ctx);
  g->self_cap = (int64_t)g->R * g->NTs;
  const size_t R = g->R, d = c.d_model, L = c.n_dec_layers, NT = g->NT;
  FW_CHECK_ARG(R <= 2048, "decode_batch * max_beam must be <= 2048 (got %zu)", R);
  FW_HIP(hipSetDevice(m->device));
  if (!lane->stream) FW_HIP(create_stream(&lane->stream, "DEC"));
  int rc;
#define A(p, n) do { if ((rc = g->bufs.alloc(&(p), (n)))) return rc; } while (0)
#define Z(p, n) do { if ((rc = g->bufs.zalloc(&(p), (n)))) return rc; } while (0)   // must start zeroed
  Z(g->slot_map, R);
  A(g->sk, L * (size_t)g->self_cap * d);
  A(g->sv, L * (size_t)g->self_cap * d);
  A(g->x, R * d); A(g->qkv, R * 3 * d); A(g->att, R * d); A(g->qc, R * d);
  A(g->ffn, R * 4 * d);
  A(g->logits, R * c.n_vocab);
  A(g->prompt_dev, NT * R); A(g->prompt_blk, NT * R);
  A(g->cur_tok, R);
  A(g->hist2, 2 * R * NT);
  A(g->cum2, 2 * R);
  A(g->kvidx2, 2 * R * NT);
  A(g->cand_val, R * 32);
  A(g->cand_tok, R * 32);
  A(g->cand_lp, R * 32);
  A(g->lphist2, 2 * R * NT);
  // per-chunk state is sized by ROWS: random sampling runs every hypothesis as its own beam-1 chunk
  A(g->done, R); A(g->n_done, 1); A(g->n_fin, R);
  A(g->fin_tok, R * FIN_CAP * NT); A(g->fin_len, R * FIN_CAP);
  A(g->fin_score, R * FIN_CAP); A(g->fin_cum, R * FIN_CAP);
  A(g->fin_lp, R * FIN_CAP * (NT + 1));
  Z(g->d_step, 1);
  A(g->no_speech, R);
  A(g->sup_bits, (size_t)LP_SUP_WORDS);
  Z(g->zero_done, R);
  const size_t R16 = (R + 15) / 16 * 16;   // whole 16-row tiles
  Z(g->ptab, R); Z(g->sot_tab, R);
  Z(g->nsp_x, R16 * d); Z(g->nsp_xf, R16 * d);
  Z(g->smp_tab, R);
  Z(g->trunc_tab, R);
  if (m->compute_type == FW_COMPUTE_INT8_FLOAT16) {
    Z(g->xq, R16 * 4 * d);
    Z(g->xs, R16);
    g->ekq.cap_rows = (int64_t)g->EB * c.n_audio_ctx;
    g->ekq.cap_elems = g->ekq.cap_rows * d;
    A(g->ekq.q, (size_t)g->ekq.cap_elems);
    A(g->ekq.scale, (size_t)g->ekq.cap_rows);
  } else {
    Z(g->x_frag, R16 * d); Z(g->att_frag, R16 * d); Z(g->ffn_frag, R16 * 4 * d); Z(g->xn_frag, R16 * d);
  }
#undef A
#undef Z
  FW_HIP(hipDeviceSynchronize());
  const char* ng = getenv("FWAMD_NO_GRAPH");   // rocprofv3 7.2 crashes on replayed graphs: profile eagerly
  g->graphs_enabled = !(ng && ng[0] == '1');
  lane->gen = ws.release();
  return FW_OK;
}

int gen_workspace_ensure(Model* m, DecodeLane* lane) {
  if (int rc = cross_pool_ensure(m, m->decode_batch)) return rc;
  if (lane->gen) return FW_OK;
  return gen_workspace_build(m, lane, lane_chunks_of(m), m->decode_self_ctx);
}

void gen_workspace_free(DecodeLane* lane) {
  delete lane->gen;   // (destroys its step graphs; its DevBufs frees the device buffers)
  lane->gen = nullptr;
}

DecodeLane::~DecodeLane() {
  if (stream) (void)hipStreamSynchronize(stream);
  gen_workspace_free(this);
  if (stream) (void)hipStreamDestroy(stream);
  if (spare) (void)hipStreamDestroy(spare);
}

// K11: cross-attention K / V^T of every decoder layer for the chunks of one encoder output, written to the chunk
// slots of pool block `blk` (held by the caller; once per encoder output as long as the block is not recycled)
// cross-K/V projections of ALL decoder layers as two launches (K, V^T) instead of two per layer (fp16; knob 6 /
// FWAMD_CROSS_KV_LAYERED=0: per layer, rounds 1-4).  The 64 per-layer GEMMs are 24 000 x 1 280 x 1 280 each: 480 tiles =
// 1.875 rounds of 256 workgroups (the last round 7/8 full) with a prologue / epilogue ramp per launch; as one launch the K
// (or V^T) projection of a 16-chunk batch is 15 360 tiles = 60 full rounds.  Same tiles, same arithmetic: the same bits.
static std::atomic<int> g_cross_kv_layered{-1};
void set_cross_kv_layered(int on) { g_cross_kv_layered.store(on ? 1 : 0); }
// element strides between consecutive decoder layers' cross.kv weights / biases when they are uniform (they are for a blob
// packed by pack_blob: every layer holds the same items at the same sizes), else 0
static bool cross_kv_strides(const Model* m, int64_t* ws, int64_t* bs) {
  const int L = m->cfg.n_dec_layers;
  if (L < 2) return false;
  const int64_t w1 = m->dec[1].ck.w - m->dec[0].ck.w, b1 = m->dec[1].ck.b - m->dec[0].ck.b;
  for (int l = 1; l < L; ++l) {
    if (m->dec[l].ck.w - m->dec[0].ck.w != l * w1 || m->dec[l].cv.w - m->dec[0].cv.w != l * w1) return false;
    if (m->dec[l].ck.b - m->dec[0].ck.b != l * b1 || m->dec[l].cv.b - m->dec[0].cv.b != l * b1) return false;
  }
  *ws = w1; *bs = b1;
  return w1 > 0;
}

static int ensure_cross_kv(Model* m, DecodeLane* lane, const Tensor* enc, int blk, bool hit) {
  if (hit) return FW_OK;
  GenWorkspace* g = lane->gen;
  CrossPool* pool = m->xpool;
  const int B = enc->B;
  const int b0 = blk * pool->EB;
  // (a failure half way leaves the block marked empty — pool_acquire did that — never pointing at partly overwritten K/V)
  const fw_config& c = m->cfg;
  const int d = c.d_model, T = c.n_audio_ctx;
  const int64_t xs = (int64_t)T * d;
  hipStream_t st = lane->stream;
  int rc;
  ProfScope ps(lane->prof, PF_CROSS_KV_GEMM, 2.0 * c.n_dec_layers * B * (double)T * d * (2.0 * d), 0, st);
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  const int kvp = pool->kvp;
  const int64_t kvs = (int64_t)d * kvp;   // one chunk's K (or V^T): H heads x kvp keys x 64
  const int64_t cls = (int64_t)pool->n_slots() * kvs;          // a layer's region of the pool
  // both land in the MFMA-fragment-major layout of the decode kernel (head_rows = kvp selects it in the
  // GEMM epilogue): K through the plain epilogue, V^T through the transposed one
  LinCall k{.in = {enc->data, d, xs}, .C = pool->ck + (size_t)b0 * kvs, .ldc = d, .c_bs = kvs, .M = T, .batch = B,
            .head_rows = kvp, .st = st};
  LinCall v{.in = k.in, .C = pool->cvt + (size_t)b0 * kvs, .ldc = kvp, .c_bs = kvs, .M = T, .batch = B, .trans = true,
            .head_rows = kvp, .st = st};
  if (i8) {
    // the encoder output is quantised once and shared by all 2L projections
    if ((rc = quantise_rows(m, enc->data, nullptr, (int64_t)B * T, d, st, g->ekq))) return rc;
    k.in = v.in = {.xq = &g->ekq};
  }
  int64_t ws = 0, bs = 0;
  if (!i8 && env_knob_on(g_cross_kv_layered, "FWAMD_CROSS_KV_LAYERED") && cross_kv_strides(m, &ws, &bs)) {
    k.n_layers = v.n_layers = c.n_dec_layers;
    k.w_ls = v.w_ls = ws; k.b_ls = v.b_ls = bs; k.c_ls = v.c_ls = cls;
    if ((rc = run_linear(m, m->dec[0].ck, k)) || (rc = run_linear(m, m->dec[0].cv, v))) return rc;
  } else for (int l = 0; l < c.n_dec_layers; ++l) {
    if (l) { k.C += cls; v.C += cls; }
    if ((rc = run_linear(m, m->dec[l].ck, k)) || (rc = run_linear(m, m->dec[l].cv, v))) return rc;
  }
  std::lock_guard<std::mutex> lk(pool->mu);
  pool->blocks[blk].enc_id = enc->id;
  pool->blocks[blk].n = B;
  return FW_OK;
}

struct StepCfg {
  int rows, kmul;      // rows processed, queries per chunk (1 for prefill, K for beam steps)
  int B;
  int pos_fixed;       // >= 0: explicit position (prefill / detect / align); -1: P-1+*d_step
  int P;
  const int* ptab = nullptr;   // decode steps of a ragged run: [B] prompt length per chunk (device), instead of P
  const int* tok;      // [rows] device
  bool need_logits;
  int nospeech_rowmul; // > 0: run the no-speech kernel on rows b*rowmul after the logits GEMM
  bool beam_tail;      // logits rules + beam update + step advance
  const int* done;     // per-chunk done flags for cross-attn early exit
  int kv_slot0 = 0;    // align: first pool slot of the call's block (its chunks are contiguous there)
  // POSITION BLOCK (prompt forward, align): blk_n > 0 — rows = B * blk_n, row = chunk * blk_n + j is position
  // pos_fixed + j of the chunk's beam slot 0, kmul = blk_n.  One pass over the decoder for blk_n positions: the weights,
  // and the chunk's cross-attention K / V^T (the dominant HBM stream), are read once for all of them.
  int blk_n = 0;
  int nospeech_off = 0; // row of the chunk's block whose logits feed the no-speech kernel
  // align extras
  const int* sel_heads_dev = nullptr;   // [n_sel_total] head ids, grouped per layer
  const int* sel_layer_off = nullptr;   // host: [L+1] offsets into sel_heads
  float* probs = nullptr; int n_sel_total = 0, n_tok = 0, tok_idx = 0;
};

#define DG(call)                                                        \
  do {                                                                  \
    if ((call) != 0) {                                                  \
      set_error("decoder gemm: unsupported shape (%s)", #call);        \
      return FW_ERUNTIME;                                               \
    }                                                                   \
  } while (0)

// position blocks for the prompt forward and align (knob 4 / FWAMD_POS_BLOCKS, default ON; 0: one position per pass,
// rounds 1-4): the same bits either way (tests/test_gpu_model.py::test_position_blocks_same_bits)
static std::atomic<int> g_pos_blocks{-1};
void set_pos_blocks(int on) { g_pos_blocks.store(on ? 1 : 0); }
// positions per block for a pass over `chunks` chunks: the workspace holds g->R rows, the cross-attention kernel takes
// <= 16 queries per chunk
static int pos_block_size(const Model* m, const GenWorkspace* g, const GenDev& gp, int chunks) {
  if (!env_knob_on(g_pos_blocks, "FWAMD_POS_BLOCKS") || chunks < 1) return 1;
  if (!fwd::self_attn_block_ok(g->NT, gp.ctx, m->cfg.d_model, gp.R)) return 1;
  return std::max(1, std::min(16, g->R / chunks));
}

// Final LayerNorm + vocabulary projection of `rows` hidden rows (x row-major, x_frag its fragment-major twin: the one the
// model's LayerNorm order reads is used) -> g->logits.  Per-row arithmetic: a row gets the same logits wherever it sits.
static int project_logits(Model* m, DecodeLane* lane, const half_t* x, const half_t* x_frag, int rows) {
  GenWorkspace* g = lane->gen;
  const fw_config& c = m->cfg;
  const int d = c.d_model;
  hipStream_t st = lane->stream;
  ProfScope ps(lane->prof, PF_DEC_LOGITS, 2.0 * rows * (double)c.n_vocab * d, 2.0 * c.n_vocab * d, st);
  if (m->compute_type == FW_COMPUTE_INT8_FLOAT16) {
    fwk::launch_quant_rows(st, x, d, m->dec_ln.g, m->dec_ln.b, g->xq, g->xs, rows, d, 1);
    DG(fwd::launch_dec_logits(st, true, g->xq, g->xs, m->logits.wq, m->logits.wscale, nullptr, nullptr, g->logits,
                              c.n_vocab, rows, c.n_vocab, d));
  } else if (m->ln_unfold >= 1) {
    fwk::launch_layernorm(st, x, m->dec_ln.g, m->dec_ln.b, g->xn_frag, rows, d, 1);
    DG(fwd::launch_dec_logits(st, false, g->xn_frag, nullptr, m->logits_p.w, nullptr, nullptr, nullptr, g->logits,
                              c.n_vocab, rows, c.n_vocab, d));
  } else {
    DG(fwd::launch_dec_logits(st, false, x_frag, nullptr, m->logits.w, nullptr, m->logits.s1, m->logits.cf, g->logits,
                              c.n_vocab, rows, c.n_vocab, d));
  }
  return FW_OK;
}

// One decoder forward over `rows` rows.  Everything that varies from step to step lives in HBM (d_step, beam
// tables), and everything a captured graph bakes in by value is part of GenDev (the graph key).
static int run_step(Model* m, DecodeLane* lane, const GenDev& gp, const StepCfg& s) {
  GenWorkspace* g = lane->gen;
  const fw_config& c = m->cfg;
  const int d = c.d_model, H = c.n_heads, T = c.n_audio_ctx, NT = g->NT;
  CrossPool* pool = m->xpool;
  const int kvp = pool->kvp;
  hipStream_t st = lane->stream;
  const int rows = s.rows;
  const bool i8 = m->compute_type == FW_COMPUTE_INT8_FLOAT16;
  {
    ProfScope ps(lane->prof, PF_DEC_MISC, 0, 0, st);
    fwd::launch_embed(st, s.tok, m->tok_emb, m->dec_pos, g->x, i8 ? nullptr : g->x_frag, rows, d, g->d_step,
                      s.pos_fixed, s.P, s.blk_n, s.ptab, s.kmul, gp.reach);
  }
  // int8_float16 (K25): the row quantiser (fused with the LayerNorm where one feeds the linear) writes the int8
  // rows fragment-major, then the int8 skinny GEMM de-quantises in its epilogue
  auto lin_q = [&](const half_t* xin, const LNW* ln, const LinearW& L, const half_t* res, half_t* outp, int act) -> int {
    fwk::launch_quant_rows(st, xin, L.K, ln ? ln->g : nullptr, ln ? ln->b : nullptr, g->xq, g->xs, rows, L.K, 1);
    return fwd::launch_dec_gemm_frag_i8(st, g->xq, g->xs, L.wq, L.wscale, L.b, res, L.N, outp, L.N, rows, L.N, L.K, act);
  };
  // fp16: xin is the fragment-major copy of the input; the residual stream is kept row-major too (residual
  // adds), the FFN hidden only fragment-major; LayerNorms are folded into qkv / cross-q / ffn1
  auto lin_f = [&](const half_t* xin_frag, const LinearW& L, const half_t* res, half_t* outp, half_t* outp_frag,
                   int act) -> int {
    return fwd::launch_dec_linear(st, fwd::DecLin{xin_frag, L.w, L.b, L.s1, L.cf, res, L.N, outp, L.N, outp_frag, rows,
                                                  L.N, L.K, act});
  };
  const int frag = i8 ? 0 : 1;
  // fp16, explicit-LayerNorm order (Model::ln_unfold == 2): the LayerNorm is its own kernel, its fp16 output (fragment-
  // major) feeds the plain weight — the rounding points of an fp16 LayerNorm followed by an fp16 GEMM
  const bool unf = !i8 && m->ln_unfold >= 2;
  auto lin_u = [&](const LNW& ln, const LinearW& L, half_t* outp, half_t* outp_frag, int act) -> int {
    fwk::launch_layernorm(st, g->x, ln.g, ln.b, g->xn_frag, rows, d, 1);
    return fwd::launch_dec_linear(st, fwd::DecLin{g->xn_frag, L.w, L.b, nullptr, nullptr, nullptr, L.N, outp, L.N,
                                                  outp_frag, rows, L.N, L.K, act});
  };
  for (int l = 0; l < c.n_dec_layers; ++l) {
    const DecLayerW& L = m->dec[l];
    // the run's own cache geometry: [layer][cache_rows slots][H][ctx][64]
    half_t* kc = g->sk + (size_t)l * gp.cache_rows * gp.ctx * d;
    half_t* vc = g->sv + (size_t)l * gp.cache_rows * gp.ctx * d;
    const half_t* ck = pool->ck + (size_t)l * pool->n_slots() * d * kvp;
    const half_t* cvt = pool->cvt + (size_t)l * pool->n_slots() * d * kvp;
    {
      ProfScope ps(lane->prof, PF_DEC_GEMM_QKV, 2.0 * rows * 3.0 * d * d, 2.0 * 3.0 * d * d, st);
      if (i8) DG(lin_q(g->x, &L.ln1, L.qkv, nullptr, g->qkv, 0));
      else if (unf) DG(lin_u(L.ln1, L.qkv_p, g->qkv, nullptr, 0));
      else DG(lin_f(g->x_frag, L.qkv, nullptr, g->qkv, nullptr, 0));
    }
    {
      ProfScope ps(lane->prof, PF_DEC_SELF_ATTN, 0, 0, st);
      fwd::launch_self_attn(st, g->qkv, d, kc, vc, NT, gp.ctx, H, g->kvidx2, gp.K, s.kmul, frag ? g->att_frag : g->att, rows,
                            g->d_step, s.pos_fixed, s.P, gp.R, frag, s.blk_n, s.ptab, gp.reach);
    }
    {
      ProfScope ps(lane->prof, PF_DEC_GEMM_DXD, 2.0 * rows * 2.0 * d * d, 2.0 * 2.0 * d * d, st);
      if (i8) {
        DG(lin_q(g->att, nullptr, L.out, g->x, g->x, 0));
        DG(lin_q(g->x, &L.ln2, L.cq, nullptr, g->qc, 0));
      } else {
        DG(lin_f(g->att_frag, L.out, g->x, g->x, g->x_frag, 0));
        if (unf) DG(lin_u(L.ln2, L.cq_p, g->qc, nullptr, 0));
        else DG(lin_f(g->x_frag, L.cq, nullptr, g->qc, nullptr, 0));
      }
    }
    if (s.probs && s.sel_layer_off[l + 1] > s.sel_layer_off[l]) {
      ProfScope ps(lane->prof, PF_DEC_MISC, 0, 0, st);
      const int off = s.sel_layer_off[l], n = s.sel_layer_off[l + 1] - off;
      fwd::launch_cross_probs(st, g->qc, d, ck + (size_t)s.kv_slot0 * d * kvp, T, kvp, s.sel_heads_dev + off, n, s.n_sel_total,
                              s.probs + (size_t)off * s.n_tok * T, s.n_tok, s.tok_idx, s.B, s.blk_n);
    }
    {
      ProfScope ps(lane->prof, PF_DEC_CROSS_ATTN, 4.0 * rows * (double)T * d, 4.0 * (s.B / gp.kv_div) * (double)T * d,
                   st);
      fwd::launch_cross_attn(st, g->qc, d, ck, cvt, T, kvp, s.kmul, frag ? g->att_frag : g->att, s.B, H, s.done,
                             gp.kv_div, frag, g->slot_map);
    }
    {
      ProfScope ps(lane->prof, PF_DEC_GEMM_DXD, 2.0 * rows * 1.0 * d * d, 2.0 * 1.0 * d * d, st);
      if (i8) DG(lin_q(g->att, nullptr, L.cout, g->x, g->x, 0));
      else DG(lin_f(g->att_frag, L.cout, g->x, g->x, g->x_frag, 0));
    }
    {
      ProfScope ps(lane->prof, PF_DEC_GEMM_FFN1, 2.0 * rows * 4.0 * d * d, 2.0 * 4.0 * d * d, st);
      if (i8) DG(lin_q(g->x, &L.ln3, L.ffn1, nullptr, g->ffn, 1));
      else if (unf) DG(lin_u(L.ln3, L.ffn1_p, nullptr, g->ffn_frag, 1));
      else DG(lin_f(g->x_frag, L.ffn1, nullptr, nullptr, g->ffn_frag, 1));
    }
    {
      ProfScope ps(lane->prof, PF_DEC_GEMM_FFN2, 2.0 * rows * 4.0 * d * d, 2.0 * 4.0 * d * d, st);
      if (i8) DG(lin_q(g->ffn, nullptr, L.ffn2, g->x, g->x, 0));
      else DG(lin_f(g->ffn_frag, L.ffn2, g->x, g->x, g->x_frag, 0));
    }
  }
  if (s.need_logits || s.beam_tail) {
    if (int rc = project_logits(m, lane, g->x, g->x_frag, rows)) return rc;
  }
  if (s.nospeech_rowmul > 0) {
    ProfScope ps(lane->prof, PF_DEC_MISC, 0, 0, st);
    fwd::launch_nospeech(st, g->logits + (size_t)s.nospeech_off * c.n_vocab, c.n_vocab, s.nospeech_rowmul,
                         c.tok_no_speech, g->no_speech, s.B);
  }
  if (s.beam_tail) {
    ProfScope ps(lane->prof, PF_DEC_SAMPLE, 0, 8.0 * rows * c.n_vocab, st);
    const bool alt = gp.n_alt > 0;   // (run_alt_ensure has sized the buffers for this run)
    // the boost comes first: the rules below see the boosted logits (run_init_state has filled the table for this run)
    if (gp.boost) fwd::launch_boost_step(st, gp, g->logits, g->boost_tab.p, g->hist2, g->d_step, g->done);
    // then the constraint: what the list does not allow is -inf before the rules look
    if (gp.constrain) fwd::launch_constrain_step(st, gp, g->logits, g->constrain_tab.p, g->hist2, g->d_step, g->done);
    fwd::launch_logits_process(st, gp, g->logits, g->sup_bits, g->hist2, g->cum2, g->d_step, g->done, g->cand_val,
                               g->cand_tok, g->cand_lp, g->smp_tab, alt ? g->alt_tok.p : nullptr,
                               alt ? g->alt_lp.p : nullptr, gp.trunc ? g->trunc_tab : nullptr);
    fwd::launch_beam_update(st, gp, g->cand_val, g->cand_tok, g->hist2, g->cum2, g->kvidx2, g->cur_tok, g->d_step,
                            g->done, g->n_done, g->n_fin, g->fin_tok, g->fin_len, g->fin_score, g->fin_cum, g->cand_lp,
                            g->lphist2, g->fin_lp, s.ptab, alt ? g->fin_path.p : nullptr);
    fwd::launch_step_advance(st, g->d_step);
  }
  return FW_OK;
}

// generated-token budget: the reference treats max_length as prompt + new tokens
// (transcribe.py:193-207). [CT2-ext] single place that decides; mirrors oracle.whisper.max_new_tokens.
static int max_new_tokens(int max_length, int P) { return std::max(0, max_length - P); }
// positions a run can reach (prompt + budget), rounded up to 8: the per-slot extent of its self-attention cache
static int run_ctx(const fw_config& c, int max_length, int P) {
  const int reach = P + max_new_tokens(std::min(max_length, c.n_text_ctx), P);
  return std::min(c.n_text_ctx, (std::max(reach, 1) + 7) / 8 * 8);
}

static int check_launch(const char* what) {
  hipError_t he = hipGetLastError();
  if (he != hipSuccess) {
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(he));
    return FW_ERUNTIME;
  }
  return FW_OK;
}

// The step graph of a run: one hipGraph per distinct GenDev (everything the captured kernels take by value, kv_div
// included) and kernel-forms epoch, kept by the lane's workspace.
static hipGraphExec_t step_graph_find(GenWorkspace* g, const GenDev& gp) {
  hipGraphExec_t exec = nullptr;
  for (GraphSlot& gs : g->graphs)
    if (gs.exec && gs.forms == fwd::kernel_forms_epoch() && memcmp(&gs.key, &gp, sizeof(gp)) == 0) {
      exec = gs.exec; gs.stamp = ++g->graph_clock;
    }
  return exec;
}
// Captures step `s` on the lane's stream, instantiates it and keeps it, in a new slot or in place of the least recently
// used one.  Null when capture or instantiation fails: the caller then launches its steps eagerly.
static hipGraphExec_t step_graph_capture(Model* m, DecodeLane* lane, const GenDev& gp, const StepCfg& s) {
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    const int rc2 = run_step(m, lane, gp, s);
    const hipError_t e2 = hipStreamEndCapture(st, &graph);
    hipGraphExec_t ne = nullptr;
    if (rc2 == FW_OK && e2 == hipSuccess && graph && hipGraphInstantiate(&ne, graph, nullptr, nullptr, 0) == hipSuccess) {
      GraphSlot* slot = nullptr;
      if (g->graphs.size() < kStepGraphSlots) { g->graphs.emplace_back(); slot = &g->graphs.back(); }
      else {   // evict the least recently used
        slot = &g->graphs[0];
        for (GraphSlot& gs : g->graphs) if (gs.stamp < slot->stamp) slot = &gs;
        if (slot->exec) (void)hipGraphExecDestroy(slot->exec);
      }
      m->grp.graph_captures.fetch_add(1);
      slot->exec = ne; slot->key = gp; slot->stamp = ++g->graph_clock; slot->forms = fwd::kernel_forms_epoch();
      exec = ne;
    }
    if (graph) (void)hipGraphDestroy(graph);
  }
  (void)hipGetLastError();
  return exec;
}

// POSITION-BLOCK FORWARD: positions 0 .. n_pos - 1 of `chunks` chunks (beam slot 0 of each), all known up front — the
// prompt forward of a decode run, the teacher-forced text of align — go through the decoder in blocks of up to 16
// positions per pass (StepCfg::blk_n; pos_block_size) instead of one position per pass.  ptok holds the tokens as
// [pos][chunk] and the caller has uploaded it to g->prompt_dev; the blocked order [block][chunk][position of the block] is
// made and uploaded here (g->prompt_blk).  fill(s, pos, nb) completes the pass's StepCfg (need_logits, the no-speech row,
// done, align's extras); after(pos, nb) launches what follows the pass.
// A block of ONE position has the layout of an unblocked pass (rows = chunks, kmul = 1, blk_n = 0) and its tokens sit at
// pos * chunks in either order, so a last block of one position needs no case of its own, and a forward of a single
// position (a two-token prompt) reads g->prompt_dev as it lies: nothing to reorder, no upload to wait for.
template <typename Fill, typename After>
static int pos_block_forward(Model* m, DecodeLane* lane, const GenDev& gp, const std::vector<int>& ptok, int n_pos, int chunks,
                             int P, const HipFail& upload_fail, Fill&& fill, After&& after) {
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  const int nbmax = pos_block_size(m, g, gp, chunks);
  const bool blocked = nbmax > 1 && n_pos > 1;
  if (blocked) {
    std::vector<int> blk_tok;
    blk_tok.reserve((size_t)n_pos * chunks);
    for (int pos = 0; pos < n_pos;) {
      const int nb = std::min(nbmax, n_pos - pos);
      for (int b = 0; b < chunks; ++b)
        for (int j = 0; j < nb; ++j) blk_tok.push_back(ptok[(size_t)(pos + j) * chunks + b]);
      pos += nb;
    }
    FW_HIP_AS(upload_fail, hipMemcpyAsync(g->prompt_blk, blk_tok.data(), blk_tok.size() * sizeof(int), hipMemcpyHostToDevice, st));
    FW_HIP_AS(upload_fail, hipStreamSynchronize(st));   // blk_tok is a local
  }
  for (int pos = 0; pos < n_pos;) {
    const int nb = blocked ? std::min(nbmax, n_pos - pos) : 1;
    StepCfg s;
    s.B = chunks; s.pos_fixed = pos; s.P = P;
    s.rows = chunks * nb; s.kmul = nb; s.blk_n = nb > 1 ? nb : 0;
    s.tok = (blocked ? g->prompt_blk : g->prompt_dev) + (size_t)pos * chunks;
    s.beam_tail = false;
    fill(s, pos, nb);
    if (int rc = run_step(m, lane, gp, s)) return rc;
    after(pos, nb);
    pos += nb;
  }
  return FW_OK;
}

// ---- one fw_generate call ------------------------------------------------------------------------------------
struct GenRequest {
  const Tensor* enc;
  const int32_t* prompts;
  const int32_t* prompt_offsets;
  int B, P;
  const fw_gen_opts* o;
  int32_t* out_ids; int32_t* out_lens; float* out_scores; float* out_no_speech;
  float* out_token_logprobs = nullptr;   // [B, num_hypotheses, max_length] | null
  float* out_end_logprobs = nullptr;     // [B, num_hypotheses] | null
  // alternatives: all four, or none with n_alt == 0 (fw_generate_alt checks).  NOT part of what must agree between the calls
  // of a run: the run records the largest n_alt of its calls, each call receives its own first n_alt entries — extraction
  // is a total order, so the first n of the top m are the top n.
  int n_alt = 0;
  int32_t* out_alt_ids = nullptr;        // [B, num_hypotheses, max_length, n_alt]
  float* out_alt_logprobs = nullptr;
  int32_t* out_end_alt_ids = nullptr;    // [B, num_hypotheses, n_alt]
  float* out_end_alt_logprobs = nullptr;
  const fw_boost* boost = nullptr;       // a non-empty boost list | null (fw_generate_boost turns an empty list into null)
  const fw_constraint* constraint = nullptr;   // a non-empty constraint list | null (likewise)
  // truncated sampling (fw_generate_trunc): the limits on this call's draws, (0, 1) = none.  Like temperature and seed they
  // need NOT agree between the calls of a run: every row reads its call's from the run's TruncRow table.
  int top_k = 0;
  float top_p = 1.0f;
  bool sampling;
  int with_ts = 1, sot_pos = -1;   // from the prompt: no <|notimestamps|> -> timestamp rules; position of <sot>
  int rc = FW_OK;
  std::string err;
  bool taken = false;   // part of a run that is being decoded (its caller waits for `done`, it must not lead another run)
  bool done = false;
};

// The run's phrase table of one kind into its lane buffer.  The buffer is allocated once, at the kind's largest table
// (max_words): the pointer a cached step graph holds never changes.
static int32_t phrase_table_to_lane(GrowBuf<int>& dst, const fw_phrase_table& t, int max_words, const char* what,
                                    hipStream_t st) {
  FW_CHECK_ARG(t.table.size() <= (size_t)max_words, "%s table of %zu words", what, t.table.size());
  if (int rc = dst.ensure(max_words)) return rc;
  FW_HIP(hipMemcpyAsync(dst.p, t.table.data(), t.table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  return FW_OK;
}

// calls that may share a decode run: same scalar options (max_length among them), same suppress list, same timestamp
// mode.  SAMPLING calls share runs among themselves only (their hypotheses are beam-1 rows of their own, num_hypotheses
// decode chunks per encoder chunk: a beam or greedy call has one); sampling_temperature and seed need NOT agree, every
// row reads its call's from the run's SmpRow table, and the same holds for top_k and top_p (fw_generate_trunc; the TruncRow
// table): a truncating call shares runs with sampling calls that truncate otherwise or not at all.  The PROMPT LENGTH and
// the <|startoftranscript|> position need not agree: a run whose calls differ in either is a RAGGED run (generate_run),
// every chunk at its own position with its own budget min(max_length, n_text_ctx) - P.
// BOOST LISTS must agree: both calls have none, or their compiled tables are byte-equal (the run walks ONE table).
// CONSTRAINT LISTS (fw_generate_constrain) likewise.
static bool mergeable(const GenRequest& a, const GenRequest& b, int n_text_ctx) {
  if (a.sampling != b.sampling) return false;
  if (!fwd::phrase_table_same(a.boost, b.boost) || !fwd::phrase_table_same(a.constraint, b.constraint)) return false;
  const fw_gen_opts &x = *a.o, &y = *b.o;
  // a call whose prompt already fills max_length decodes nothing (and may lie beyond the run's cache extent): it shares
  // a run only with calls of its own prompt length and <sot> position, as before
  if ((a.P != b.P || a.sot_pos != b.sot_pos) && std::max(a.P, b.P) >= std::min(x.max_length, n_text_ctx)) return false;
  if (x.beam_size != y.beam_size || x.patience != y.patience || x.num_hypotheses != y.num_hypotheses ||
      x.length_penalty != y.length_penalty || x.repetition_penalty != y.repetition_penalty ||
      x.no_repeat_ngram_size != y.no_repeat_ngram_size || x.max_length != y.max_length ||
      x.max_initial_timestamp_index != y.max_initial_timestamp_index || x.suppress_blank != y.suppress_blank ||
      x.min_new_tokens != y.min_new_tokens || x.n_suppress_tokens != y.n_suppress_tokens)
    return false;
  if (x.n_suppress_tokens && memcmp(x.suppress_tokens, y.suppress_tokens, x.n_suppress_tokens * sizeof(int32_t)))
    return false;
  // the timestamp rules are switched by <|notimestamps|> in the prompt: that must agree; the prompts themselves may
  // differ (language token per chunk, transcribe.py:212-220; previous text of any length in front of <sot>)
  return a.with_ts == b.with_ts;
}

// share (percent) of a run's capacity an IDLE decode group (no run in progress) waits for; FWAMD_IDLE_FILL_PCT overrides
static int idle_fill_pct() {
  static const int v = [] {
    const char* e = getenv("FWAMD_IDLE_FILL_PCT");
    const int x = e ? atoi(e) : 100;
    return x < 1 ? 1 : (x > 100 ? 100 : x);
  }();
  return v;
}
// an idle two-lane group splits the known work evenly over its runs (leader_stops_gathering); FWAMD_IDLE_BALANCE=0 turns it
// off (the A/B of profiles/r05_ab_idle_balance.jsonl: burst 2 904 -> 2 976x, steady state 3 105 -> 3 105x)
static bool idle_balance() {
  static const bool v = [] { const char* e = getenv("FWAMD_IDLE_BALANCE"); return !e || atoi(e) != 0; }();
  return v;
}
// chunks an IDLE two-lane group wants queued before it leads a run: its even share of the work it knows of — `queued`
// chunks in `n_queued` requests plus one request of that average size per worker inside an encode call — over the runs
// that work needs (at least two: one per lane; more when it exceeds two runs' capacity `want`), never less than one batch
// (round 6: splitting the known work of an idle group into at least THREE runs instead of two — the first run starting after a
//  third of a burst's encoder passes — measured +-0.4 % on the 20-batch burst and on the steady state: profiles/r06_ab_idle_runs.jsonl)
int64_t idle_lead_chunks(int64_t queued, int n_queued, int encoding, int64_t want, int max_batch, int lanes) {
  const int64_t per_req = std::max<int64_t>(1, queued / std::max<int64_t>(1, (int64_t)n_queued));
  const int64_t outstanding = queued + (int64_t)std::max(0, encoding) * per_req;
  const int64_t n_runs = std::max<int64_t>(std::max(2, lanes), (outstanding + std::max<int64_t>(1, want) - 1) / std::max<int64_t>(1, want));
  return std::max<int64_t>(max_batch, (outstanding + n_runs - 1) / n_runs);
}

// What a lane holds of runs led by a call of `B` chunks — THE statement of run capacity: the entry check of fw_generate,
// the leader's wait (leader_wait), the gather loop (take_mergeable) and generate_run's workspace checks all read it.  The lane: `lane_chunks` chunks x
// `max_beam` rows and a self-attention cache of `self_cap` row-positions (its planned size before the workspace exists,
// the workspace's own in generate_run); the call: beam_size / num_hypotheses and ctx = run_ctx() of its max_length
// (mergeable calls share max_length, hence the context).
RunCapacity::RunCapacity(int lane_chunks, int max_batch, int max_beam, int64_t self_cap_, int B, bool sampling, int beam_size,
                         int num_hypotheses, int ctx_) {
  // rows of one encoder chunk in the run: beam_size, or num_hypotheses beam-1 rows when sampling (kv_div)
  rows_per_chunk = sampling ? std::max(1, num_hypotheses) : beam_size;
  rows = (int64_t)B * rows_per_chunk;
  row_cap = (int64_t)lane_chunks * max_beam;
  self_cap = self_cap_;
  ctx = ctx_;
  rows_fit = rows <= row_cap;
  cache_fits = rows * ctx <= self_cap;
  // the rows above which the 4 x 4-tile decoder linears no longer fit the chip in one round of workgroups
  // (d x d: 20 column groups x 25 row groups of 64 rows = 500 of 512 workgroup slots)
  const int64_t one_round = std::max<int64_t>(max_batch, DEC_RUN_MAX_ROWS / std::max(1, beam_size));
  // (the leader of a run of SAMPLING calls does not wait for further ones: fallback attempts are stragglers)
  want =sampling ? 0 : std::min<int64_t>(lane_chunks, one_round);
  // chunks the self-attention cache holds at this context, never less than the leading call itself ...
  run_cap = std::min<int64_t>(lane_chunks, std::max<int64_t>(B, self_cap / std::max<int64_t>(1, rows_per_chunk * ctx)));
  if (!sampling)
    run_cap = std::min(run_cap, one_round);
  else   // ... num_hypotheses rows per chunk, not bounded by max_beam: the run's rows must fit the lane's
    run_cap = std::min(run_cap, std::max<int64_t>(B, (int64_t)lane_chunks * max_beam / std::max(1, num_hypotheses)));
}
// ... of a lane of `dm` as planned (the workspace may not exist yet), for runs led by `r`
static RunCapacity planned_capacity(const Model* dm, const GenRequest& r) {
  const int B = lane_chunks_of(dm);
  const int nts = self_positions(dm, B, dm->decode_self_ctx > 0 ? dm->decode_self_ctx : dm->cfg.n_text_ctx);
  // (rows x positions of a lane's self-attention cache)
  return RunCapacity(B, dm->max_batch, dm->max_beam, (int64_t)B * dm->max_beam * nts, r.B, r.sampling, r.o->beam_size,
                     r.o->num_hypotheses, run_ctx(dm->cfg, r.o->max_length, r.P));
}

// ---- a decode run over the concatenated chunks of `reqs` (all mergeable with reqs[0]), phase by phase; generate_run
//      below strings the phases together.  Every phase runs under lane->mu on the lane's stream. ----
struct RunPlan {
  const fw_gen_opts* o;       // the leading call's options (mergeable calls agree on all that the run reads from them)
  bool sampling, ragged, want_nsp;
  int K, nh, ml;              // beam_size, num_hypotheses, max_length
  int P, Pmax;                // shortest and longest prompt of the run
  int B, Bx, kv_div;          // encoder chunks, decode chunks = B * kv_div, decode chunks per encoder chunk
  int budget, ctx, reach, sot_pos;
  GenDev gp;                  // what the step kernels take by value: the step graph's key
};

// Phase 1: the run's geometry, checked against the workspace, and its GenDev.
static int run_plan(const Model* m, const GenWorkspace* g, const std::vector<GenRequest*>& reqs, RunPlan& pl) {
  const fw_config& c = m->cfg;
  const GenRequest& r0 = *reqs[0];
  const fw_gen_opts* o = pl.o = r0.o;
  const int K = pl.K = o->beam_size;
  const bool sampling = pl.sampling = r0.sampling;
  // RAGGED run: its calls differ in prompt length or <sot> position (mergeable() lets them meet).  They share
  // reach = min(max_length, n_text_ctx), hence the cache geometry; chunk c has its own prompt length P_c and its own budget
  // reach - P_c.  P is the SHORTEST prompt (the run lasts reach - P steps), Pmax the longest (the prompt forward runs to
  // Pmax - 1).  A uniform run (P == Pmax, one <sot> position) takes exactly the path it always took.
  pl.P = pl.Pmax = r0.P; pl.B = 0; pl.ragged = pl.want_nsp = false;
  int n_alt = 0;   // the largest of the run's calls: what the run records (0: nothing, the kernels and graph keys of always)
  bool trunc = false;   // some call of the run limits its draw (sampling calls only: fw_generate_trunc checks)
  for (const GenRequest* r : reqs) {
    pl.P = std::min(pl.P, r->P); pl.Pmax = std::max(pl.Pmax, r->P);
    pl.ragged = pl.ragged || r->P != r0.P || r->sot_pos != r0.sot_pos;
    pl.want_nsp = pl.want_nsp || r->o->return_no_speech_prob;
    pl.B += r->B;
    n_alt = std::max(n_alt, r->n_alt);
    trunc = trunc || r->top_k > 0 || r->top_p < 1.0f;
  }
  pl.nh = o->num_hypotheses; pl.ml = o->max_length;
  const int P = pl.P, Pmax = pl.Pmax, B = pl.B;
  const bool ragged = pl.ragged;
  const int kv_div = pl.kv_div = sampling ? pl.nh : 1;
  const int Bx = pl.Bx = B * kv_div;
  const int budget = pl.budget = max_new_tokens(std::min(o->max_length, c.n_text_ctx), P);
  const int ctx = pl.ctx = run_ctx(c, o->max_length, P);
  const int reach = pl.reach = std::min(o->max_length, c.n_text_ctx);
  // the whole run against the REAL workspace: its rows (= Bx * K; the per-chunk tables ptab / sot_tab / nsp_x hold one
  // entry per decode chunk, g->R of them, and Bx <= Bx * K), its chunks and its cache
  const RunCapacity cap(g->B, g->EB, g->K, g->self_cap, B, sampling, K, pl.nh, ctx);
  FW_CHECK_ARG(cap.rows_fit && B <= g->B, "decode run of %d chunks x %d rows exceeds the workspace", B, kv_div * K);
  // (every position a ragged run touches lies below reach <= ctx: mergeable() keeps prompts that fill max_length out)
  FW_CHECK_ARG(!ragged || Pmax < reach, "ragged decode run: prompt of %d tokens with max_length %d", Pmax, pl.ml);
  FW_CHECK_ARG(cap.cache_fits, "decode run of %d rows x %d positions exceeds the self-attention cache", Bx * K, ctx);
  GenDev& gp = pl.gp;
  memset(&gp, 0, sizeof(gp));
  // (ragged: the step kernels read neither P nor budget — zero in the key, so that ragged runs of one size share a graph
  //  whatever their prompt lengths)
  gp.B = Bx; gp.K = K; gp.R = Bx * K; gp.P = ragged ? 0 : P; gp.budget = ragged ? 0 : budget; gp.kv_div = kv_div;
  gp.ctx = ctx; gp.cache_rows = Bx * K;
  gp.ragged = ragged ? 1 : 0; gp.reach = ragged ? reach : 0;   // (part of the step graph's key)
  gp.sample = sampling ? 1 : 0;
  gp.n_alt = n_alt;
  gp.boost = r0.boost ? 1 : 0;   // (mergeable calls agree on the list)
  gp.constrain = r0.constraint ? 1 : 0;   // (likewise)
  gp.trunc = (sampling && trunc) ? 1 : 0;   // (a run without a truncating call: today's kernels and graphs)
  // temperature and seed are per CALL: a sampling run reads them from g->smp_tab (filled below), a run of one call
  // included, and they stay out of the step graph's key — sampling runs of one size share a graph whatever their seeds
  gp.inv_temp = 1.0f; gp.seed_lo = 0; gp.seed_hi = 0;
  gp.max_fin = std::max(1, (int)lroundf((float)K * o->patience));
  if (gp.max_fin > FIN_CAP - K) gp.max_fin = FIN_CAP - K;
  gp.V = c.n_vocab; gp.n_text_ctx = g->NT;
  pl.sot_pos = r0.sot_pos;   // (uniform runs; a ragged run reads each chunk's own, see the prompt forward)
  fwd::fill_rule_fields(gp, c, o, r0.with_ts);
  gp.lp_pow = o->length_penalty;
  return FW_OK;
}

// Alternatives: the lane's buffers for a run that records n_alt > 0 per row and step, allocated by the first such run and
// grown by replacement when a later one needs more (the lane is idle: its mutex is held and its stream was waited for).  A
// cached step graph holds the old pointers: the graphs that record alternatives go with them.  Runs that record none
// allocate nothing and touch nothing here.
static int run_alt_ensure(DecodeLane* lane, const RunPlan& pl) {
  GenWorkspace* g = lane->gen;
  if (pl.gp.n_alt <= 0) return FW_OK;
  const int64_t n_alt = (int64_t)pl.budget * pl.gp.R * pl.gp.n_alt;
  const int64_t n_path = (int64_t)g->R * FIN_CAP * (g->NT + 1);
  if (n_alt > g->alt_tok.cap || n_alt > g->alt_lp.cap || n_path > g->fin_path.cap) {
    FW_HIP(hipStreamSynchronize(lane->stream));
    for (GraphSlot& gs : g->graphs)
      if (gs.exec && gs.key.n_alt > 0) { (void)hipGraphExecDestroy(gs.exec); gs.exec = nullptr; gs.stamp = 0; }
    int rc;
    if ((rc = g->alt_tok.ensure(n_alt)) || (rc = g->alt_lp.ensure(n_alt)) || (rc = g->fin_path.ensure(n_path))) return rc;
  }
  return FW_OK;
}

// Phase 2: the run's blocks of the cross-attention pool (all at once; `hold` keeps them to the end of the run), the
// projection of those that are not there yet, and the run's table encoder chunk -> pool slot (slots: [B], host).
static int run_acquire_blocks(Model* m, DecodeLane* lane, const std::vector<GenRequest*>& reqs, PoolHold& hold,
                              std::vector<int>& slots) {
  CrossPool* pool = m->xpool;
  std::vector<uint64_t> ids;
  std::vector<int> ns;
  std::vector<char> hit;
  for (const GenRequest* r : reqs) { ids.push_back(r->enc->id); ns.push_back(r->enc->B); }
  FW_CHECK_ARG((int)reqs.size() <= pool->n_blocks, "decode run of %zu calls exceeds the %d blocks of the cross-attention pool",
               reqs.size(), pool->n_blocks);
  pool_acquire(pool, ids, ns, hold.blk, hit);
  for (size_t i = 0; i < reqs.size(); ++i) {
    if (int rc = ensure_cross_kv(m, lane, reqs[i]->enc, hold.blk[i], hit[i] != 0)) return rc;
    for (int b = 0; b < reqs[i]->B; ++b) slots.push_back(hold.blk[i] * pool->EB + b);
  }
  return FW_OK;
}

// Phase 3: state init (only the rows of this run) and the host tables: suppress mask, prompts, first-step tokens, the
// ragged / sampling tables, the slot table.  ptok: the prompt tokens as [pos][decode chunk], for the prompt forward.
static int run_init_state(Model* m, DecodeLane* lane, const std::vector<GenRequest*>& reqs, const RunPlan& pl,
                          const std::vector<int>& slots, std::vector<int>& ptok) {
  GenWorkspace* g = lane->gen;
  const fw_config& c = m->cfg;
  hipStream_t st = lane->stream;
  const fw_gen_opts* o = pl.o;
  const bool sampling = pl.sampling, ragged = pl.ragged;
  const int K = pl.K, Pmax = pl.Pmax, B = pl.B, Bx = pl.Bx, kv_div = pl.kv_div;
  // (the ping-pong halves of hist2 / kvidx2 / cum2 are gp.R rows apart: the kernels index them with the run's R)
  const size_t NT = g->NT, Rr = (size_t)pl.gp.R;
  FW_HIP(hipMemsetAsync(g->hist2, 0, 2 * Rr * NT * sizeof(int), st));
  FW_HIP(hipMemsetAsync(g->lphist2, 0, 2 * Rr * NT * sizeof(float), st));
  FW_HIP(hipMemsetAsync(g->kvidx2, 0, 2 * Rr * NT, st));
  FW_HIP(hipMemsetAsync(g->cum2, 0, 2 * Rr * sizeof(float), st));
  FW_HIP(hipMemsetAsync(g->done, 0, Rr * sizeof(int), st));
  FW_HIP(hipMemsetAsync(g->n_done, 0, sizeof(int), st));
  FW_HIP(hipMemsetAsync(g->n_fin, 0, Rr * sizeof(int), st));
  FW_HIP(hipMemsetAsync(g->d_step, 0, sizeof(int), st));
  FW_HIP(hipMemsetAsync(g->no_speech, 0, Rr * sizeof(float), st));
  const std::vector<unsigned long long> mask = fwd::suppress_mask(o->suppress_tokens, o->n_suppress_tokens, c.n_vocab);
  FW_HIP(hipMemcpyAsync(g->sup_bits, mask.data(), mask.size() * sizeof(mask[0]), hipMemcpyHostToDevice, st));
  if (pl.gp.boost)
    if (int rc = phrase_table_to_lane(g->boost_tab, *reqs[0]->boost, fwd::BOOST_TABLE_MAX_WORDS, "boost", st)) return rc;
  if (pl.gp.constrain)
    if (int rc = phrase_table_to_lane(g->constrain_tab, *reqs[0]->constraint, fwd::CONSTRAIN_TABLE_MAX_WORDS, "constraint", st))
      return rc;
  // prompt tokens transposed to [pos][bx]; first-step tokens replicated per beam.  Ragged: positions at and beyond a
  // chunk's last prompt token are padded with that token (see the prompt forward)
  ptok.assign((size_t)Pmax * Bx, 0);
  std::vector<int> first((size_t)Bx * K), ptab_host((size_t)Bx), sot_host((size_t)Bx);
  std::vector<fwd::SmpRow> smp_host(sampling ? (size_t)Bx : 0);   // (sampling: K == 1, decode chunk bx is row bx)
  std::vector<fwd::TruncRow> trunc_host(pl.gp.trunc ? (size_t)Bx : 0);
  {
    int bx = 0;
    for (const GenRequest* r : reqs) {
      const int row0 = bx;   // first row of this call: its rows draw their noise as rows 0 .. of a run of their own
      for (int b = 0; b < r->B; ++b)
        for (int j = 0; j < kv_div; ++j, ++bx) {
          const int32_t* pr = r->prompts + r->prompt_offsets[b];
          for (int p = 0; p < Pmax; ++p) ptok[(size_t)p * Bx + bx] = pr[std::min(p, r->P - 1)];
          for (int k = 0; k < K; ++k) first[(size_t)bx * K + k] = pr[r->P - 1];
          ptab_host[bx] = r->P; sot_host[bx] = r->sot_pos;
          if (sampling)
            smp_host[bx] = {1.0f / r->o->sampling_temperature, (unsigned)(r->o->seed & 0xffffffffu),
                            (unsigned)(r->o->seed >> 32), row0};
          if (pl.gp.trunc) trunc_host[bx] = {r->top_k, r->top_p};
        }
    }
  }
  if (sampling)
    FW_HIP(hipMemcpyAsync(g->smp_tab, smp_host.data(), (size_t)Bx * sizeof(fwd::SmpRow), hipMemcpyHostToDevice, st));
  if (pl.gp.trunc)
    FW_HIP(hipMemcpyAsync(g->trunc_tab, trunc_host.data(), (size_t)Bx * sizeof(fwd::TruncRow), hipMemcpyHostToDevice, st));
  if (ragged) {
    FW_HIP(hipMemcpyAsync(g->ptab, ptab_host.data(), (size_t)Bx * sizeof(int), hipMemcpyHostToDevice, st));
    FW_HIP(hipMemcpyAsync(g->sot_tab, sot_host.data(), (size_t)Bx * sizeof(int), hipMemcpyHostToDevice, st));
  }
  FW_HIP(hipMemcpyAsync(g->prompt_dev, ptok.data(), ptok.size() * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP(hipMemcpyAsync(g->cur_tok, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, st));
  // (the cross-attention kernel divides the decode chunk by kv_div before it looks the slot up: one entry per ENCODER chunk)
  FW_HIP(hipMemcpyAsync(g->slot_map, slots.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP(hipStreamSynchronize(st));   // the host buffers above are locals
  return FW_OK;
}

// Phase 4: prompt forward (all but the last token): Bx rows, beam slot 0 of every chunk, in position blocks
//      (pos_block_forward: one pass for the 3 positions of the usual 4-token prompt; a prompt that carries 223 tokens of
//      previous text takes 14 passes instead of 223)
//      RAGGED run: the passes run to Pmax - 1 with ALL chunks in every pass.  Chunk c is really there only while
//      pos < P_c - 1; in later passes it rides along on padding (its own last prompt token).  That is harmless: a padded
//      row reads only its own chunk's cache slot and sibling rows, and what it writes — K / V of beam slot 0 at positions
//      >= P_c - 1, all below reach, inside the slot — is written again by the chunk's real decode steps before anything
//      reads it: step s writes position P_c - 1 + s on every beam slot and reads only positions below it.  Its valid rows
//      (positions < P_c - 1) see exactly what they see in a run of their own, so the chunk's bits do not change.
//      The no-speech probability is read at each chunk's own <sot> position: the final hidden row there is gathered into
//      a Bx-row buffer as its pass (or step 0) goes by, and ONE vocabulary projection follows step 0.
static int run_prompt_forward(Model* m, DecodeLane* lane, const RunPlan& pl, const std::vector<int>& ptok) {
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  int rc = pos_block_forward(
      m, lane, pl.gp, ptok, pl.Pmax - 1, pl.Bx, pl.Pmax, HipFail{FW_ENODEV, "prompt forward: token upload"},
      [&](StepCfg& s, int pos, int nb) {
        s.need_logits = !pl.ragged && pl.sot_pos >= pos && pl.sot_pos < pos + nb && pl.want_nsp;
        s.nospeech_rowmul = s.need_logits ? nb : 0;
        s.nospeech_off = s.need_logits ? pl.sot_pos - pos : 0;
        s.done = g->done;
      },
      [&](int pos, int nb) {
        if (pl.ragged && pl.want_nsp)
          fwd::launch_gather_sot_rows(st, g->x, g->sot_tab, g->ptab, pos, nb, nb, g->nsp_x, g->nsp_xf, m->cfg.d_model, pl.Bx);
      });
  if (rc) return rc;
  return check_launch("prompt forward");
}

// Phase 5: step 0, eagerly, then one step-graph replay per step until every chunk is done or the budget is spent.
static int run_decode_steps(Model* m, DecodeLane* lane, const RunPlan& pl) {
  GenWorkspace* g = lane->gen;
  const fw_config& c = m->cfg;
  hipStream_t st = lane->stream;
  const GenDev& gp = pl.gp;
  const bool ragged = pl.ragged, want_nsp = pl.want_nsp;
  const int K = pl.K, P = pl.P, Bx = pl.Bx, budget = pl.budget, sot_pos = pl.sot_pos;
  int rc;
  int steps_done = 0;
  if (budget > 0) {
    // ---- step 0 (eager): last prompt token on all rows; beams are identical copies ----
    StepCfg s;
    s.rows = Bx * K; s.kmul = K; s.B = Bx; s.pos_fixed = -1; s.P = P; s.tok = g->cur_tok;
    s.ptab = ragged ? g->ptab : nullptr;
    s.need_logits = true;
    s.nospeech_rowmul = (!ragged && sot_pos == P - 1 && want_nsp) ? K : 0;
    s.beam_tail = true;
    s.done = g->done;
    if ((rc = run_step(m, lane, gp, s))) return rc;
    steps_done = 1;
    s.nospeech_rowmul = 0;
    if (ragged && want_nsp) {
      // the chunks whose prompt ENDS with <sot> had their row in step 0 (g->x still holds its final hidden state); then one
      // projection over the Bx gathered rows — g->logits is free between two steps
      fwd::launch_gather_sot_rows(st, g->x, g->sot_tab, g->ptab, 0, 0, K, g->nsp_x, g->nsp_xf, c.d_model, Bx);
      if ((rc = project_logits(m, lane, g->nsp_x, g->nsp_xf, Bx))) return rc;
      ProfScope ps(lane->prof, PF_DEC_MISC, 0, 0, st);
      fwd::launch_nospeech(st, g->logits, c.n_vocab, 1, c.tok_no_speech, g->no_speech, Bx);
    }

    // ---- steps 1.. : one hipGraph replay per step; graphs are cached per GenDev (everything the captured
    //      kernels take by value, kv_div included) ----
    hipGraphExec_t exec = nullptr;
    if (g->graphs_enabled && !lane->prof.on) {
      exec = step_graph_find(g, gp);
      if (!exec) exec = step_graph_capture(m, lane, gp, s);
    }
    int n_done_host = 0;
    while (steps_done < budget) {
      const int burst = std::min(4, budget - steps_done);
      for (int i = 0; i < burst; ++i) {
        if (exec) {
          hipError_t he = hipGraphLaunch(exec, st);
          if (he != hipSuccess) {
            set_error("hipGraphLaunch failed: %s", hipGetErrorString(he));
            return FW_ERUNTIME;
          }
        } else if ((rc = run_step(m, lane, gp, s))) {
          return rc;
        }
      }
      steps_done += burst;
      FW_HIP(hipMemcpyAsync(&n_done_host, g->n_done, sizeof(int), hipMemcpyDeviceToHost, st));
      FW_HIP(hipStreamSynchronize(st));
      if (n_done_host >= Bx) break;
    }
  }
  FW_HIP(hipStreamSynchronize(st));
  if ((rc = check_launch("decode loop"))) return rc;
  prof_collect(lane->prof);
  return FW_OK;
}

// Phase 6: finalize on the host: the best num_hypotheses of every encoder chunk by normalised score (stable), into the
// output buffers of the chunk's call.
static int run_finalize(DecodeLane* lane, const std::vector<GenRequest*>& reqs, const RunPlan& pl) {
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  const bool ragged = pl.ragged;
  const int Bx = pl.Bx, kv_div = pl.kv_div, nh = pl.nh, ml = pl.ml;
  const size_t NT = g->NT;
  std::vector<int> n_fin(Bx), fin_len((size_t)Bx * FIN_CAP);
  std::vector<float> fin_score((size_t)Bx * FIN_CAP), nsp(Bx);
  std::vector<int> fin_tok((size_t)Bx * FIN_CAP * NT);
  // (on the decode stream, not the legacy default stream: a default-stream copy would wait for every blocking
  //  stream of the device)
  FW_HIP(hipMemcpyAsync(n_fin.data(), g->n_fin, Bx * sizeof(int), hipMemcpyDeviceToHost, st));
  FW_HIP(hipMemcpyAsync(fin_len.data(), g->fin_len, fin_len.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  FW_HIP(hipMemcpyAsync(fin_score.data(), g->fin_score, fin_score.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  FW_HIP(hipMemcpyAsync(fin_tok.data(), g->fin_tok, fin_tok.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  FW_HIP(hipMemcpyAsync(nsp.data(), g->no_speech, Bx * sizeof(float), hipMemcpyDeviceToHost, st));
  // the per-token log-probs are recorded by every run; they come back only when a request of this one asked
  bool want_lp = false;
  for (const GenRequest* r : reqs) want_lp = want_lp || r->out_token_logprobs || r->out_end_logprobs;
  std::vector<float> fin_lp;
  if (want_lp) {
    fin_lp.resize((size_t)Bx * FIN_CAP * (NT + 1));
    FW_HIP(hipMemcpyAsync(fin_lp.data(), g->fin_lp, fin_lp.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  FW_HIP(hipStreamSynchronize(st));
  // alternatives: the returned hypotheses of the calls that asked, in the order they are met below; one gather launch
  // after the selection, then every call copies its own first n_alt of the run's
  std::vector<fwd::AltHyp> alt_hyps;
  std::vector<std::pair<GenRequest*, size_t>> alt_dst;
  const int n_alt_run = pl.gp.n_alt, alt_T = pl.budget;
  int cb = 0;   // first chunk of the request inside the run
  for (GenRequest* r : reqs) {
    for (int b = 0; b < r->B; ++b) {
      const int gb = cb + b;
      // (ragged: a prompt without <sot> has no gathered row — 0, as in a run of its own)
      if (r->o->return_no_speech_prob) r->out_no_speech[b] = (ragged && r->sot_pos < 0) ? 0.f : nsp[(size_t)gb * kv_div];
      // candidate hypotheses of encoder chunk gb: (decode chunk, finished index)
      std::vector<std::pair<int, int>> hyps;
      for (int j = 0; j < kv_div; ++j) {
        const int bx = gb * kv_div + j;
        for (int f = 0; f < n_fin[bx]; ++f) hyps.push_back({bx, f});
      }
      std::stable_sort(hyps.begin(), hyps.end(), [&](const std::pair<int, int>& a, const std::pair<int, int>& bb) {
        return fin_score[(size_t)a.first * FIN_CAP + a.second] > fin_score[(size_t)bb.first * FIN_CAP + bb.second];
      });
      for (int h = 0; h < nh && h < (int)hyps.size(); ++h) {
        const size_t f = (size_t)hyps[h].first * FIN_CAP + hyps[h].second;
        int len = fin_len[f];
        if (len > ml) len = ml;
        r->out_lens[b * nh + h] = len;
        if (r->o->return_scores) r->out_scores[b * nh + h] = fin_score[f];
        memcpy(r->out_ids + ((size_t)b * nh + h) * ml, &fin_tok[f * NT], (size_t)len * sizeof(int));
        if (r->out_token_logprobs)
          memcpy(r->out_token_logprobs + ((size_t)b * nh + h) * ml, &fin_lp[f * (NT + 1)], (size_t)len * sizeof(float));
        if (r->out_end_logprobs) r->out_end_logprobs[b * nh + h] = fin_lp[f * (NT + 1) + NT];
        if (r->n_alt > 0) {
          // recorded on <eot> at step fin_len < the chunk's budget, or cut at the last step with fin_len == budget
          const int budget_c = max_new_tokens(std::min(ml, (int)NT), r->P);
          alt_hyps.push_back({hyps[h].first, hyps[h].second, len, fin_len[f] < budget_c ? fin_len[f] : -1});
          alt_dst.push_back({r, (size_t)b * nh + h});
        }
      }
    }
    cb += r->B;
  }
  if (alt_hyps.empty()) return FW_OK;
  const int n_hyp = (int)alt_hyps.size();
  const size_t per_hyp = (size_t)(alt_T + 1) * n_alt_run;
  int rc;
  if ((rc = g->alt_hyps.ensure(n_hyp)) || (rc = g->alt_out_tok.ensure((int64_t)(n_hyp * per_hyp))) ||
      (rc = g->alt_out_lp.ensure((int64_t)(n_hyp * per_hyp))))
    return rc;
  std::vector<int> a_tok(n_hyp * per_hyp);
  std::vector<float> a_lp(n_hyp * per_hyp);
  FW_HIP(hipMemcpyAsync(g->alt_hyps.p, alt_hyps.data(), n_hyp * sizeof(fwd::AltHyp), hipMemcpyHostToDevice, st));
  fwd::launch_alt_gather(st, g->alt_tok.p, g->alt_lp.p, g->fin_path.p, g->alt_hyps.p, n_hyp, pl.gp.R, pl.K, (int)NT,
                         n_alt_run, alt_T, g->alt_out_tok.p, g->alt_out_lp.p);
  FW_HIP(hipMemcpyAsync(a_tok.data(), g->alt_out_tok.p, a_tok.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  FW_HIP(hipMemcpyAsync(a_lp.data(), g->alt_out_lp.p, a_lp.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  FW_HIP(hipStreamSynchronize(st));
  if ((rc = check_launch("alternatives gather"))) return rc;
  for (size_t ih = 0; ih < alt_hyps.size(); ++ih) {   // hypothesis ih belongs to slot alt_dst[ih] of its call
    GenRequest* r = alt_dst[ih].first;
    const size_t slot = alt_dst[ih].second;   // b * nh + h
    const int n = r->n_alt, len = alt_hyps[ih].len;
    const int* stok = &a_tok[ih * per_hyp];
    const float* slp = &a_lp[ih * per_hyp];
    for (int t = 0; t <= len; ++t) {   // t == len: the end slot, row alt_T of the gather's output
      const size_t src = (size_t)(t < len ? t : alt_T) * n_alt_run;
      int32_t* oi = t < len ? r->out_alt_ids + (slot * ml + t) * n : r->out_end_alt_ids + slot * n;
      float* ol = t < len ? r->out_alt_logprobs + (slot * ml + t) * n : r->out_end_alt_logprobs + slot * n;
      for (int j = 0; j < n; ++j) { oi[j] = stok[src + j]; ol[j] = slp[src + j]; }
    }
  }
  return FW_OK;
}

// Decode run over the concatenated chunks of `reqs` (all mergeable with reqs[0]).  Caller holds lane->mu.
static int generate_run(Model* m, DecodeLane* lane, const std::vector<GenRequest*>& reqs) {
  int rc = gen_workspace_ensure(m, lane);
  if (rc) return rc;
  RunPlan pl;
  if ((rc = run_plan(m, lane->gen, reqs, pl))) return rc;
  FW_HIP(hipSetDevice(m->device));
  PoolHold hold{m->xpool, {}, lane->stream};
  std::vector<int> slots, ptok;
  if ((rc = run_alt_ensure(lane, pl))) return rc;
  if ((rc = run_acquire_blocks(m, lane, reqs, hold, slots))) return rc;
  if ((rc = run_init_state(m, lane, reqs, pl, slots, ptok))) return rc;
  if ((rc = run_prompt_forward(m, lane, pl, ptok))) return rc;
  if ((rc = run_decode_steps(m, lane, pl))) return rc;
  return run_finalize(lane, reqs, pl);
}

// ---- the run scheduler of a decode group.  A caller of fw_generate queues its request and, when no one else is gathering
//      and a lane is free, LEADS the next run: leader_wait, take_mergeable, run_on_free_lane. ----

// Should the leader of the next run stop waiting for further requests?  Policy only: every value was read under grp.mu.
// `queued` chunks in `n_queued` requests; `encoding` member encodes in flight (requests about to arrive); `lanes` that may
// run (fw_model_set_decode_lanes); `want` chunks a run led by the oldest request takes (RunCapacity); fill_pct: the share
// of `want` at which the leader stops (fw_model_set_merge_wait); wait_over: the newest request arrived longer ago than
// the merge wait.
static bool leader_stops_gathering(int64_t queued, int n_queued, int encoding, int active_runs, int lanes, int64_t want,
                                   int max_batch, int fill_pct, bool wait_over) {
  // no run in progress at all: every further request waited for is decode time the chip spends idle on the HBM
  // side (the encoders are MFMA-bound), so an idle group leads with a smaller share of a run's capacity
  // (idle_fill_pct(): the driver's 20-step burst was ONE run of 288 chunks after 18 serial encoder passes plus two
  // runs of 16 chunks; with 50 % it is two runs of 160 chunks, the second gathered under the first)
  const int pct = active_runs == 0 ? std::min(fill_pct, idle_fill_pct()) : fill_pct;
  if (queued * 100 >= want * pct || encoding <= 0) return true;
  // ... and with two lanes it splits the work it KNOWS of evenly over the runs that work needs: what is queued plus
  // one request per worker that is inside an encode call (running or waiting for the encoder; counted at the size of
  // the queued requests).  20 batches in flight -> two runs of 10, not one of 18 and leftovers.
  if (idle_balance() && active_runs == 0 && lanes >= 2 &&
      queued >= idle_lead_chunks(queued, n_queued, encoding, want, max_batch, lanes))
    return true;
  return wait_over;
}

// The leader's wait: for the requests of workers that are still encoding (each arrives within one encoder pass) unless
// most of a run's capacity is already claimed.  The wait trades this caller's latency for rows per run; it is bounded by
// the merge-wait knob (fw_model_set_merge_wait: default 2.5 measured encoder passes after the last arrival, at most
// 250 ms — a pass next to a decode run takes up to twice the pass the average was taken from, and a leader that
// gives up between two arrivals starts a run of one or two batches: the driver's 20-step burst 2 976 -> 3 030x with
// 150 or 250 ms, the steady state unchanged, profiles/r05_ab_idle_balance.jsonl; 0 = never) and skipped when no
// member encode is in flight.
// Locking: called with grp.mu held through `lk` and grp.gathering set by the caller (one caller gathers at a time); the
// mutex is released only inside the timed waits, so requests keep arriving, and is held again on return.
static void leader_wait(Model* dm, std::unique_lock<std::mutex>& lk) {
  DecodeGroup& grp = dm->grp;
  int wait_ms = grp.merge_wait_ms.load();
  if (wait_ms < 0) wait_ms = std::min(250, std::max(5, (grp.enc_pass_us.load() * 5 / 2 + 999) / 1000));
  if (lane_chunks_of(dm) <= dm->max_batch || wait_ms <= 0) return;
  for (;;) {
    const int64_t want = planned_capacity(dm, *grp.queue.front()).want;
    if (want <= 0) return;   // (the oldest request is a sampling call)
    int64_t queued = 0;
    for (const GenRequest* r : grp.queue) queued += r->B;
    const bool wait_over = std::chrono::steady_clock::now() - grp.last_arrival > std::chrono::milliseconds(wait_ms);
    if (leader_stops_gathering(queued, (int)grp.queue.size(), grp.encoding.load(), grp.active_runs,
                               std::min((int)dm->lanes.size(), grp.lanes_enabled.load()), want, dm->max_batch,
                               grp.merge_fill_pct.load(), wait_over))
      return;
    grp.cv.wait_for(lk, std::chrono::microseconds(200));
  }
}

// Takes the oldest request and every queued request that can share a run with it off the queue (marked `taken`), up to
// the run's capacity and one pool block per call; returns the run's chunks.  Locking: grp.mu held throughout.
static int take_mergeable(Model* dm, std::vector<GenRequest*>& batch) {
  DecodeGroup& grp = dm->grp;
  GenRequest* first = grp.queue.front();
  const int64_t run_cap = planned_capacity(dm, *first).run_cap;
  const int max_calls = pool_block_count(dm->decode_batch, dm->max_batch);
  int chunks = 0;
  for (auto it = grp.queue.begin(); it != grp.queue.end();) {
    GenRequest* r = *it;
    if (r == first || (mergeable(*first, *r, dm->cfg.n_text_ctx) && chunks + r->B <= run_cap && (int)batch.size() < max_calls)) {
      batch.push_back(r);
      r->taken = true;
      chunks += r->B;
      it = grp.queue.erase(it);
    } else {
      ++it;
    }
  }
  return chunks;
}

// Runs `batch` (`chunks` chunks) on the first free lane and hands every request its result.  Locking: called with grp.mu
// held through `lk` and a lane free (active_runs < lanes); takes the lane and ends the caller's gathering under the mutex,
// RELEASES it for the run itself (which holds the lane's own mutex; the next leader may gather while this run decodes)
// and holds it again on return, the requests done and the lane free.
static void run_on_free_lane(Model* dm, std::unique_lock<std::mutex>& lk, const std::vector<GenRequest*>& batch, int chunks) {
  DecodeGroup& grp = dm->grp;
  const int n_lanes = (int)dm->lanes.size();
  int lane = 0;
  while (lane + 1 < n_lanes && dm->lanes[lane]->busy) ++lane;    // the first free lane (active_runs < lanes: one is)
  DecodeLane* dl = dm->lanes[lane].get();    // own workspace, own stream; the weights and the pool are dm's
  dl->busy = true;
  grp.active_runs += 1;
  grp.gathering = false;
  grp.cv.notify_all();
  lk.unlock();
  grp.n_runs.fetch_add(1);
  grp.n_requests.fetch_add((int64_t)batch.size());
  grp.n_chunks.fetch_add(chunks);
  if (chunks > grp.max_run_chunks.load()) grp.max_run_chunks.store(chunks);
  int rc;
  // FWAMD_RUN_LOG=1: one stderr line per decode run (start / end on the host clock, lane, calls, chunks) — the timeline of a
  // burst (profiles/r06_run_log_burst.txt)
  static const bool run_log = [] { const char* e = getenv("FWAMD_RUN_LOG"); return e && atoi(e) != 0; }();
  const auto t_run0 = std::chrono::steady_clock::now();
  {
    std::lock_guard<std::mutex> run_lk(dl->mu);
    rc = generate_run(dm, dl, batch);
  }
  if (run_log) {
    const auto t_run1 = std::chrono::steady_clock::now();
    const double s0 = std::chrono::duration<double>(t_run0.time_since_epoch()).count();
    const double s1 = std::chrono::duration<double>(t_run1.time_since_epoch()).count();
    int p_lo = batch[0]->P, p_hi = batch[0]->P;
    for (const GenRequest* r : batch) { p_lo = std::min(p_lo, r->P); p_hi = std::max(p_hi, r->P); }
    fprintf(stderr, "[fwamd run] lane %d calls %d chunks %d prompt %d..%d start %.4f end %.4f (%.1f ms)\n", lane,
            (int)batch.size(), chunks, p_lo, p_hi, s0, s1, 1e3 * (s1 - s0));
  }
  const std::string err = rc ? fw_last_error() : "";
  lk.lock();
  for (GenRequest* r : batch) { r->rc = rc; r->err = err; r->done = true; }
  dl->busy = false;
  grp.active_runs -= 1;
  grp.cv.notify_all();
}

// ---- a single teacher-forced call on lane 0 (fw_detect_language, fw_align): one encoder output, every position known ----
struct SingleCall {
  std::vector<int> slots;    // [B] pool slots of its chunks (contiguous); outlives `hold`, whose end waits for the upload
  PoolHold hold{nullptr, {}, nullptr};   // the call's pool block, to the end of the call
  GenDev gp;
};
// Takes the pool block of `enc` (projecting its cross-K/V if it is not there), uploads the slot table, clears the beam
// tables that a teacher-forced pass reads (kvidx2: every row reads its own cache slot; d_step) and fills the GenDev of
// P positions with `ctx` cache positions per row; builds the lane's workspace on first use.  Caller holds lane->mu and
// waits for the stream before `sc` goes.
static int single_call_begin(Model* m, DecodeLane* lane, const Tensor* enc, int P, int ctx, const HipFail& fail, SingleCall& sc) {
  FW_HIP(hipSetDevice(m->device));
  if (int rc = gen_workspace_ensure(m, lane)) return rc;
  GenWorkspace* g = lane->gen;
  const int B = enc->B;
  hipStream_t st = lane->stream;
  CrossPool* pool = m->xpool;
  sc.hold.p = pool; sc.hold.st = st;
  std::vector<char> hit;
  pool_acquire(pool, {enc->id}, {enc->B}, sc.hold.blk, hit);
  if (int rc = ensure_cross_kv(m, lane, enc, sc.hold.blk[0], hit[0] != 0)) return rc;
  sc.slots.resize(B);
  for (int b = 0; b < B; ++b) sc.slots[b] = sc.hold.blk[0] * pool->EB + b;
  FW_HIP_AS(fail, hipMemcpyAsync(g->slot_map, sc.slots.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(fail, hipMemsetAsync(g->kvidx2, 0, 2 * (size_t)g->R * g->NT, st));
  FW_HIP_AS(fail, hipMemsetAsync(g->d_step, 0, sizeof(int), st));
  GenDev& gp = sc.gp;
  memset(&gp, 0, sizeof(gp));
  // rows of a prefill-style step use beam slot 0 of chunk b: slot stride is max_beam
  gp.B = B; gp.K = m->max_beam; gp.R = g->R; gp.P = P; gp.V = m->cfg.n_vocab; gp.n_text_ctx = g->NT; gp.kv_div = 1;
  gp.ctx = ctx; gp.cache_rows = B * m->max_beam;   // <= EB * K * NT <= self_cap
  return FW_OK;
}

}  // namespace fw

using namespace fw;

extern "C" {

int32_t fw_generate(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                    int32_t B, const fw_gen_opts* o, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                    float* out_no_speech) {
  return fw_generate_lp(fm, enc_t, prompts, prompt_offsets, B, o, out_ids, out_lens, out_scores, out_no_speech, nullptr,
                        nullptr);
}

int32_t fw_generate_lp(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                       int32_t B, const fw_gen_opts* o, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                       float* out_no_speech, float* out_token_logprobs, float* out_end_logprobs) {
  return fw_generate_alt(fm, enc_t, prompts, prompt_offsets, B, o, 0, out_ids, out_lens, out_scores, out_no_speech,
                         out_token_logprobs, out_end_logprobs, nullptr, nullptr, nullptr, nullptr);
}

int32_t fw_generate_alt(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                        int32_t B, const fw_gen_opts* o, int32_t n_alt, int32_t* out_ids, int32_t* out_lens,
                        float* out_scores, float* out_no_speech, float* out_token_logprobs, float* out_end_logprobs,
                        int32_t* out_alt_ids, float* out_alt_logprobs, int32_t* out_end_alt_ids,
                        float* out_end_alt_logprobs) {
  return fw_generate_boost(fm, enc_t, prompts, prompt_offsets, B, o, n_alt, nullptr, out_ids, out_lens, out_scores,
                           out_no_speech, out_token_logprobs, out_end_logprobs, out_alt_ids, out_alt_logprobs,
                           out_end_alt_ids, out_end_alt_logprobs);
}

int32_t fw_generate_boost(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                          int32_t B, const fw_gen_opts* o, int32_t n_alt, const fw_boost* boost, int32_t* out_ids,
                          int32_t* out_lens, float* out_scores, float* out_no_speech, float* out_token_logprobs,
                          float* out_end_logprobs, int32_t* out_alt_ids, float* out_alt_logprobs,
                          int32_t* out_end_alt_ids, float* out_end_alt_logprobs) {
  return fw_generate_trunc(fm, enc_t, prompts, prompt_offsets, B, o, 0, 1.0f, n_alt, boost, out_ids, out_lens, out_scores,
                           out_no_speech, out_token_logprobs, out_end_logprobs, out_alt_ids, out_alt_logprobs,
                           out_end_alt_ids, out_end_alt_logprobs);
}

int32_t fw_generate_trunc(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                          int32_t B, const fw_gen_opts* o, int32_t top_k, float top_p, int32_t n_alt,
                          const fw_boost* boost, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                          float* out_no_speech, float* out_token_logprobs, float* out_end_logprobs,
                          int32_t* out_alt_ids, float* out_alt_logprobs, int32_t* out_end_alt_ids,
                          float* out_end_alt_logprobs) {
  return fw_generate_constrain(fm, enc_t, prompts, prompt_offsets, B, o, top_k, top_p, n_alt, boost, nullptr, out_ids,
                               out_lens, out_scores, out_no_speech, out_token_logprobs, out_end_logprobs, out_alt_ids,
                               out_alt_logprobs, out_end_alt_ids, out_end_alt_logprobs);
}

// What fw_generate_constrain and fw_score_constrain refuse (include/fwamd.h): a list for another vocabulary, and rules
// under which a listed phrase cannot be reached or a row is left without a live id.  `o`: the call's options / the scoring
// rules; check_min_new: generate only (scoring does not read min_new_tokens).
static int32_t constraint_check(const fw_constraint* ct, const fw_config& c, const fw_gen_opts* o, bool check_min_new) {
  FW_CHECK_ARG(ct->n_vocab == c.n_vocab, "the constraint list was built for a vocabulary of %d ids, the model has %d",
               ct->n_vocab, c.n_vocab);
  if (!fwd::phrase_list_live(ct)) return FW_OK;   // (an empty list: no constraint, nothing to refuse)
  FW_CHECK_ARG(c.tok_eot >= 0 && c.tok_eot < c.tok_timestamp_begin && c.tok_timestamp_begin <= c.n_vocab &&
                   c.n_vocab <= LP_SUP_WORDS * 64,
               "this model's vocabulary layout (<eot> %d, first timestamp %d, %d ids) is not one the constraint kernel takes",
               c.tok_eot, c.tok_timestamp_begin, c.n_vocab);
  FW_CHECK_ARG(o->no_repeat_ngram_size <= 0, "a constraint list does not go with no_repeat_ngram_size %d: a listed phrase "
               "that repeats an n-gram would be unreachable", o->no_repeat_ngram_size);
  FW_CHECK_ARG(!check_min_new || o->min_new_tokens <= 0, "a constraint list does not go with min_new_tokens %d: a row "
               "whose phrase is complete would have no live id", o->min_new_tokens);
  const std::vector<unsigned long long> mask = fwd::suppress_mask(o->suppress_tokens, o->n_suppress_tokens, c.n_vocab);
  const fwd::ConstrainView cv = fwd::constrain_view(ct->table.data());
  for (int j = 0; j < cv.P; ++j)
    for (int i = cv.off[j]; i < cv.off[j + 1]; ++i) {
      const int t = cv.tok[i];
      FW_CHECK_ARG(t < c.tok_eot, "constraint phrase %d holds id %d: phrases are text, ids below <eot> = %d", ct->first[j], t,
                   c.tok_eot);
      FW_CHECK_ARG(!((mask[t >> 6] >> (t & 63)) & 1ull), "constraint phrase %d holds id %d, which the suppress list forbids",
                   ct->first[j], t);
      if (i == cv.off[j] && o->suppress_blank)
        for (int k = 0; k < c.n_suppress_begin; ++k)
          FW_CHECK_ARG(t != c.suppress_begin[k], "constraint phrase %d starts with id %d, which suppress_blank forbids at "
                       "the first step", ct->first[j], t);
    }
  return FW_OK;
}

int32_t fw_generate_constrain(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                              int32_t B, const fw_gen_opts* o, int32_t top_k, float top_p, int32_t n_alt,
                              const fw_boost* boost, const fw_constraint* constraint, int32_t* out_ids, int32_t* out_lens,
                              float* out_scores, float* out_no_speech, float* out_token_logprobs, float* out_end_logprobs,
                              int32_t* out_alt_ids, float* out_alt_logprobs, int32_t* out_end_alt_ids,
                              float* out_end_alt_logprobs) {
  FW_CHECK_ARG(fm && enc_t && prompts && prompt_offsets && o && out_ids && out_lens && out_scores && out_no_speech,
               "null argument");
  FW_CHECK_ARG(n_alt >= 0 && n_alt <= FW_MAX_ALTERNATIVES, "n_alt %d not in [0, %d]", n_alt, FW_MAX_ALTERNATIVES);
  if (n_alt == 0)
    FW_CHECK_ARG(!out_alt_ids && !out_alt_logprobs && !out_end_alt_ids && !out_end_alt_logprobs,
                 "n_alt == 0 takes no alternative arrays");
  else
    FW_CHECK_ARG(out_alt_ids && out_alt_logprobs && out_end_alt_ids && out_end_alt_logprobs,
                 "n_alt > 0 needs all four alternative arrays");
  Model* m = &fm->impl;
  Model* dm = decoder_of(m);
  const Tensor* enc = &enc_t->impl;
  const fw_config& c = m->cfg;
  FW_CHECK_ARG(decoder_of(*enc) == dm, "encoder output belongs to a different model");
  FW_CHECK_ARG(B == enc->B, "batch %d does not match the encoder output batch %d", B, enc->B);
  FW_CHECK_ARG(B >= 1 && B <= dm->max_batch, "batch %d exceeds max_batch %d", B, dm->max_batch);
  FW_CHECK_ARG(!boost || boost->n_vocab == c.n_vocab, "the boost list was built for a vocabulary of %d ids, the model has %d",
               boost ? boost->n_vocab : 0, c.n_vocab);
  if (constraint)
    if (int rc = constraint_check(constraint, c, o, true)) return rc;
  const int K = o->beam_size;
  FW_CHECK_ARG(K >= 1 && K <= dm->max_beam, "beam_size %d not in [1, max_beam=%d]", K, dm->max_beam);
  // random sampling (the sequential path's temperature fallback, transcribe.py:1433-1439): beam_size 1,
  // sampling_topk 0 (whole distribution), num_hypotheses = best_of independent samples per chunk
  const bool sampling = (K == 1 && o->sampling_topk != 1);
  FW_CHECK_ARG(top_k >= 0, "top_k %d must not be negative", top_k);
  FW_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "top_p %g not in (0, 1]", (double)top_p);   // (NaN fails both)
  FW_CHECK_ARG((top_k == 0 && top_p == 1.f) || (sampling && o->sampling_topk == 0),
               "top_k / top_p limit a sampled draw: the call must sample (beam_size 1, sampling_topk 0)");
  if (sampling) {
    FW_CHECK_ARG(o->sampling_topk == 0, "sampling_topk must be 1 (greedy) or 0 (sample the whole distribution)");
    FW_CHECK_ARG(o->sampling_temperature > 0.f, "sampling_temperature must be positive");
    FW_CHECK_ARG(o->num_hypotheses >= 1, "num_hypotheses must be positive");
  } else {
    FW_CHECK_ARG(o->num_hypotheses >= 1 && o->num_hypotheses <= std::max(K, 1),
                 "num_hypotheses %d must be in [1, beam_size]", o->num_hypotheses);
  }
  FW_CHECK_ARG(o->patience > 0.f, "patience must be positive");
  FW_CHECK_ARG(o->max_length >= 1, "max_length must be positive");
  const int P = prompt_offsets[1] - prompt_offsets[0];
  FW_CHECK_ARG(P >= 1, "prompts must not be empty");
  for (int b = 0; b < B; ++b)
    FW_CHECK_ARG(prompt_offsets[b + 1] - prompt_offsets[b] == P,
                 "all prompts of a generate() call must have the same length (prompt %d has %d tokens, expected %d)",
                 b, prompt_offsets[b + 1] - prompt_offsets[b], P);
  FW_CHECK_ARG(P <= c.n_text_ctx, "prompt length %d exceeds the text context %d", P, c.n_text_ctx);
  for (int i = 0; i < B * P; ++i)
    FW_CHECK_ARG(prompts[prompt_offsets[0] + i] >= 0 && prompts[prompt_offsets[0] + i] < c.n_vocab,
                 "prompt token %d out of range", prompts[prompt_offsets[0] + i]);
  const int nh = o->num_hypotheses;
  for (int i = 0; i < B * nh; ++i) { out_lens[i] = 0; out_scores[i] = 0.f; }
  for (int b = 0; b < B; ++b) out_no_speech[b] = 0.f;
  if (out_token_logprobs) std::fill(out_token_logprobs, out_token_logprobs + (size_t)B * nh * o->max_length, 0.f);
  if (out_end_logprobs) std::fill(out_end_logprobs, out_end_logprobs + (size_t)B * nh, 0.f);
  if (n_alt > 0) {   // (id -1, log-prob 0): entries past a hypothesis' length, and the end slot of one cut at the budget
    const size_t n_tok = (size_t)B * nh * o->max_length * n_alt, n_end = (size_t)B * nh * n_alt;
    std::fill(out_alt_ids, out_alt_ids + n_tok, -1);
    std::fill(out_alt_logprobs, out_alt_logprobs + n_tok, 0.f);
    std::fill(out_end_alt_ids, out_end_alt_ids + n_end, -1);
    std::fill(out_end_alt_logprobs, out_end_alt_logprobs + n_end, 0.f);
  }

  GenRequest req;
  req.enc = enc; req.prompts = prompts; req.prompt_offsets = prompt_offsets; req.B = B; req.P = P; req.o = o;
  req.out_ids = out_ids; req.out_lens = out_lens; req.out_scores = out_scores; req.out_no_speech = out_no_speech;
  req.out_token_logprobs = out_token_logprobs; req.out_end_logprobs = out_end_logprobs;
  req.n_alt = n_alt; req.out_alt_ids = out_alt_ids; req.out_alt_logprobs = out_alt_logprobs;
  req.out_end_alt_ids = out_end_alt_ids; req.out_end_alt_logprobs = out_end_alt_logprobs;
  req.sampling = sampling;
  req.top_k = top_k; req.top_p = top_p;
  req.boost = fwd::phrase_list_live(boost) ? boost : nullptr;   // (an empty list does nothing: the call is a plain one)
  req.constraint = fwd::phrase_list_live(constraint) ? constraint : nullptr;   // (likewise)
  for (int b = 0; b < B; ++b) {
    // every prompt of the call must agree on what switches the decoding rules (true for every call site of the
    // reference: one prompt per batch, language token swapped in place)
    int wt = 1, sp = -1;
    for (int i = 0; i < P; ++i) {
      const int t = prompts[prompt_offsets[b] + i];
      if (t == c.tok_no_timestamps) wt = 0;
      if (t == c.tok_sot) sp = i;
    }
    if (b == 0) { req.with_ts = wt; req.sot_pos = sp; }
    FW_CHECK_ARG(wt == req.with_ts && sp == req.sot_pos,
                 "the prompts of a generate() call must agree on <|notimestamps|> and on the <|startoftranscript|> position");
  }

  DecodeGroup& grp = dm->grp;
  std::unique_lock<std::mutex> lk(grp.mu);
  // fw_model_set_decode_batch rebuilds the workspaces and the lanes under grp.resizing: nothing is read from
  // them (capacities, dm->lanes) and nothing is queued until it is done
  while (grp.resizing) grp.cv.wait(lk);
  // this call alone must fit a lane (rows and self-attention cache), so that a call that cannot is refused here,
  // before it is merged with others whose run it would fail
  const RunCapacity cap = planned_capacity(dm, req);
  if (!cap.rows_fit || !cap.cache_fits) {
    lk.unlock();
    set_error("this call needs %lld decoder rows x %d positions; a decode run of this model holds %lld rows and %lld "
              "row-positions (batch x num_hypotheses / beam_size too large for max_length %d)",
              (long long)cap.rows, cap.ctx, (long long)cap.row_cap, (long long)cap.self_cap, o->max_length);
    return FW_EINVAL;
  }
  grp.queue.push_back(&req);
  grp.last_arrival = std::chrono::steady_clock::now();
  while (!req.done) {
    const int n_lanes = (int)dm->lanes.size();       // (read under grp.mu: stable while a request is queued, see above)
    if (req.taken || grp.gathering || grp.active_runs >= std::min(n_lanes, grp.lanes_enabled.load())) {
      grp.cv.wait(lk);
      continue;
    }
    // lead the next run: the OLDEST request and what merges with it (if this caller's own is not among them, it goes round
    // again).  With two lanes the next leader starts gathering as soon as this one has gone off to run its requests.
    grp.gathering = true;
    leader_wait(dm, lk);
    std::vector<GenRequest*> batch;
    const int chunks = take_mergeable(dm, batch);
    run_on_free_lane(dm, lk, batch, chunks);
  }
  lk.unlock();
  if (req.rc) set_error("%s", req.err.c_str());
  return req.rc;
}

int32_t fw_detect_language(fw_model* fm, const fw_tensor* enc_t, int32_t B, int32_t* out_lang_ids,
                           float* out_probs) {
  FW_CHECK_ARG(fm && enc_t && out_lang_ids && out_probs, "null argument");
  Model* m = decoder_of(&fm->impl);
  const Tensor* enc = &enc_t->impl;
  const fw_config& c = m->cfg;
  FW_CHECK_ARG(c.is_multilingual && c.n_langs > 0, "detect_language needs a multilingual model");
  FW_CHECK_ARG(decoder_of(*enc) == m && B == enc->B && B <= m->max_batch,
               "bad encoder output / batch");
  DecodeLane* lane = m->lanes[0].get();
  std::lock_guard<std::mutex> lk(lane->mu);
  int rc;
  SingleCall sc;
  if ((rc = single_call_begin(m, lane, enc, 1, 8, HipFail{FW_ENODEV, "detect_language setup"}, sc))) return rc;
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  std::vector<int> tok(B, c.tok_sot);
  FW_HIP(hipMemcpyAsync(g->prompt_dev, tok.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP(hipStreamSynchronize(st));
  StepCfg s;
  s.rows = B; s.kmul = 1; s.B = B; s.pos_fixed = 0; s.P = 1; s.tok = g->prompt_dev;
  s.need_logits = true; s.nospeech_rowmul = 0; s.beam_tail = false; s.done = g->zero_done;
  if ((rc = run_step(m, lane, sc.gp, s))) return rc;
  std::vector<float> lg((size_t)B * c.n_langs);
  FW_HIP(hipMemcpy2DAsync(lg.data(), c.n_langs * sizeof(float), g->logits + c.tok_lang_begin,
                          (size_t)c.n_vocab * sizeof(float), c.n_langs * sizeof(float), B, hipMemcpyDeviceToHost, st));
  FW_HIP(hipStreamSynchronize(st));
  if ((rc = check_launch("detect_language"))) return rc;
  prof_collect(lane->prof);
  for (int b = 0; b < B; ++b) {
    const float* r = &lg[(size_t)b * c.n_langs];
    float mx = r[0];
    for (int i = 1; i < c.n_langs; ++i) mx = std::max(mx, r[i]);
    std::vector<float> p(c.n_langs);
    float sum = 0.f;
    for (int i = 0; i < c.n_langs; ++i) { p[i] = expf(r[i] - mx); sum += p[i]; }
    for (int i = 0; i < c.n_langs; ++i) p[i] /= sum;
    std::vector<int> order(c.n_langs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int bb) { return p[a] > p[bb]; });
    for (int i = 0; i < c.n_langs; ++i) {
      out_lang_ids[(size_t)b * c.n_langs + i] = c.tok_lang_begin + order[i];
      out_probs[(size_t)b * c.n_langs + i] = p[order[i]];
    }
  }
  return FW_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// align: standardise over tokens, median filter over frames, mean over heads (device),
// DTW (host, like CTranslate2).
// ------------------------------------------------------------------------------------
__global__ void align_stats_kernel(const float* __restrict__ probs, int n_sel, int n_tok_cap, int T,
                                   const int* __restrict__ n_tok, const int* __restrict__ nfr,
                                   float* __restrict__ stats) {
  const int b = blockIdx.z, hs = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nfr[b]) return;
  const int n = n_tok[b];
  const float* p = probs + (((size_t)b * n_sel + hs) * n_tok_cap) * T + t;
  float mean = 0.f;
  for (int i = 0; i < n; ++i) mean += p[(size_t)i * T];
  mean /= (float)n;
  float var = 0.f;
  for (int i = 0; i < n; ++i) {
    const float dlt = p[(size_t)i * T] - mean;
    var += dlt * dlt;
  }
  var /= (float)n;
  float* so = stats + (((size_t)b * n_sel + hs) * T + t) * 2;
  so[0] = mean;
  so[1] = 1.0f / sqrtf(var);
}

__global__ void align_filter_kernel(const float* __restrict__ probs, const float* __restrict__ stats, int n_sel,
                                    int n_tok_cap, int T, const int* __restrict__ n_tok, const int* __restrict__ nfr,
                                    int width, float* __restrict__ out) {
  const int b = blockIdx.z, tok = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int F = nfr[b];
  if (t >= F || tok >= n_tok[b]) return;
  const int pad = width / 2;
  float acc = 0.f;
  for (int hs = 0; hs < n_sel; ++hs) {
    const float* p = probs + (((size_t)b * n_sel + hs) * n_tok_cap + tok) * T;
    const float* st = stats + ((size_t)b * n_sel + hs) * T * 2;
    float w[15];
    const bool filt = pad > 0 && F > pad;
    const int wd = filt ? width : 1;
    for (int i = 0; i < wd; ++i) {
      int tt = filt ? t - pad + i : t;
      if (tt < 0) tt = -tt;                    // reflect padding
      if (tt >= F) tt = 2 * (F - 1) - tt;
      w[i] = (p[tt] - st[2 * tt]) * st[2 * tt + 1];
    }
    for (int i = 1; i < wd; ++i) {             // insertion sort (width <= 15)
      const float v = w[i];
      int q = i - 1;
      while (q >= 0 && w[q] > v) { w[q + 1] = w[q]; --q; }
      w[q + 1] = v;
    }
    acc += w[filt ? pad : 0];
  }
  out[((size_t)b * n_tok_cap + tok) * T + t] = acc / (float)n_sel;
}

namespace fw {
void launch_align_post(hipStream_t st, const float* probs, float* stats, int n_sel, int n_tok_cap, int T, int B,
                       const int* n_tok, const int* nfr, int width, float* mat) {
  dim3 g1((T + 127) / 128, n_sel, B);
  align_stats_kernel<<<g1, 128, 0, st>>>(probs, n_sel, n_tok_cap, T, n_tok, nfr, stats);
  dim3 g2((T + 127) / 128, n_tok_cap, B);
  align_filter_kernel<<<g2, 128, 0, st>>>(probs, stats, n_sel, n_tok_cap, T, n_tok, nfr, width, mat);
}

// openai-whisper timing.dtw_cpu on cost = -matrix (N text rows x M frames)
static void dtw_path(const float* mat, int ld, int N, int M, std::vector<int>& ti, std::vector<int>& fi) {
  std::vector<double> D((size_t)(N + 1) * (M + 1), INFINITY);
  std::vector<int8_t> tr((size_t)(N + 1) * (M + 1), -1);
  auto at = [&](int i, int j) -> size_t { return (size_t)i * (M + 1) + j; };
  D[at(0, 0)] = 0;
  for (int j = 1; j <= M; ++j)
    for (int i = 1; i <= N; ++i) {
      const double c0 = D[at(i - 1, j - 1)], c1 = D[at(i - 1, j)], c2 = D[at(i, j - 1)];
      double cc; int8_t t;
      if (c0 < c1 && c0 < c2) { cc = c0; t = 0; }
      else if (c1 < c0 && c1 < c2) { cc = c1; t = 1; }
      else { cc = c2; t = 2; }
      D[at(i, j)] = -(double)mat[(size_t)(i - 1) * ld + (j - 1)] + cc;
      tr[at(i, j)] = t;
    }
  for (int j = 0; j <= M; ++j) tr[at(0, j)] = 2;
  for (int i = 0; i <= N; ++i) tr[at(i, 0)] = 1;
  int i = N, j = M;
  ti.clear(); fi.clear();
  while (i > 0 || j > 0) {
    ti.push_back(i - 1); fi.push_back(j - 1);
    const int8_t t = tr[at(i, j)];
    if (t == 0) { --i; --j; }
    else if (t == 1) { --i; }
    else { --j; }
  }
  std::reverse(ti.begin(), ti.end());
  std::reverse(fi.begin(), fi.end());
}
}  // namespace fw

extern "C" int32_t fw_align(fw_model* fm, const fw_tensor* enc_t, const int32_t* start_seq, int32_t n_start,
                            const int32_t* text_tokens, const int32_t* text_offsets, const int32_t* num_frames,
                            int32_t B, int32_t median_filter_width, int32_t max_pairs, int32_t* out_pairs,
                            int32_t* out_n_pairs, float* out_probs) {
  FW_CHECK_ARG(fm && enc_t && start_seq && text_tokens && text_offsets && num_frames && out_pairs && out_n_pairs &&
                   out_probs, "null argument");
  Model* m = decoder_of(&fm->impl);
  const Tensor* enc = &enc_t->impl;
  const fw_config& c = m->cfg;
  FW_CHECK_ARG(decoder_of(*enc) == m && B == enc->B && B <= m->max_batch,
               "bad encoder output / batch");
  FW_CHECK_ARG(n_start >= 1, "start_sequence must not be empty");
  FW_CHECK_ARG(median_filter_width >= 1 && median_filter_width <= 15 && (median_filter_width & 1),
               "median_filter_width must be odd and <= 15");
  const int T = c.n_audio_ctx, d = c.d_model;
  // teacher-forced sequences: start + no_timestamps + text + eot
  std::vector<std::vector<int>> seq(B);
  int max_tok = 0;
  for (int b = 0; b < B; ++b) {
    const int nt = text_offsets[b + 1] - text_offsets[b];
    FW_CHECK_ARG(nt >= 0, "bad text offsets");
    for (int i = 0; i < n_start; ++i) seq[b].push_back(start_seq[i]);
    seq[b].push_back(c.tok_no_timestamps);
    for (int i = 0; i < nt; ++i) {
      const int t = text_tokens[text_offsets[b] + i];
      FW_CHECK_ARG(t >= 0 && t < c.n_vocab, "text token %d out of range", t);
      seq[b].push_back(t);
    }
    seq[b].push_back(c.tok_eot);
    FW_CHECK_ARG((int)seq[b].size() <= c.n_text_ctx, "align sequence of %zu tokens exceeds the text context", seq[b].size());
    max_tok = std::max(max_tok, (int)seq[b].size());
  }
  // alignment heads grouped per layer
  std::vector<std::vector<int>> per_layer(c.n_dec_layers);
  if (c.n_align_heads > 0) {
    for (int i = 0; i < c.n_align_heads; ++i) {
      const int l = c.align_heads[2 * i], h = c.align_heads[2 * i + 1];
      FW_CHECK_ARG(l >= 0 && l < c.n_dec_layers && h >= 0 && h < c.n_heads, "alignment head (%d,%d) out of range", l, h);
      per_layer[l].push_back(h);
    }
  } else {  // [CT2-ext] default: all heads of the upper half of the decoder
    for (int l = c.n_dec_layers / 2; l < c.n_dec_layers; ++l)
      for (int h = 0; h < c.n_heads; ++h) per_layer[l].push_back(h);
  }
  std::vector<int> sel_heads, layer_off(c.n_dec_layers + 1, 0);
  for (int l = 0; l < c.n_dec_layers; ++l) {
    layer_off[l] = (int)sel_heads.size();
    for (int h : per_layer[l]) sel_heads.push_back(h);
  }
  layer_off[c.n_dec_layers] = (int)sel_heads.size();
  const int n_sel = (int)sel_heads.size();
  FW_CHECK_ARG(n_sel > 0, "no alignment heads");

  DecodeLane* lane = m->lanes[0].get();
  std::lock_guard<std::mutex> lk(lane->mu);
  int rc;
  const HipFail setup_fail{FW_ERUNTIME, "align setup"}, run_fail{FW_ERUNTIME, "align"};
  // teacher forcing: every position is known up front (<= EB * K * NT row-positions of the cache: <= self_cap)
  SingleCall sc;
  if ((rc = single_call_begin(m, lane, enc, max_tok, std::min(c.n_text_ctx, (max_tok + 7) / 8 * 8), setup_fail, sc))) return rc;
  GenWorkspace* g = lane->gen;
  hipStream_t st = lane->stream;
  const int kv_slot0 = sc.slots[0];

  DevBufs tmp;   // (after `sc`: freed before the pool block is released)
  float *probs = nullptr, *stats = nullptr, *mat = nullptr, *tprob = nullptr;
  int *heads_dev = nullptr, *ntok_dev = nullptr, *nfr_dev = nullptr, *target_dev = nullptr;
  if ((rc = tmp.alloc(&probs, (size_t)B * n_sel * max_tok * T)) || (rc = tmp.alloc(&stats, (size_t)B * n_sel * T * 2)) ||
      (rc = tmp.alloc(&mat, (size_t)B * max_tok * T)) || (rc = tmp.alloc(&tprob, (size_t)B * max_tok)) ||
      (rc = tmp.alloc(&heads_dev, (size_t)n_sel)) || (rc = tmp.alloc(&ntok_dev, (size_t)B)) ||
      (rc = tmp.alloc(&nfr_dev, (size_t)B)) || (rc = tmp.alloc(&target_dev, (size_t)max_tok * B)))
    return rc;
  std::vector<int> ntok(B), nfr(B), ptok((size_t)max_tok * B), target((size_t)max_tok * B, -1);
  for (int b = 0; b < B; ++b) {
    ntok[b] = (int)seq[b].size();
    nfr[b] = std::min(T, std::max(1, num_frames[b] / 2));
    for (int p = 0; p < max_tok; ++p) {
      ptok[(size_t)p * B + b] = p < ntok[b] ? seq[b][p] : c.tok_eot;
      // the logits at position p predict token p+1; we want probs of the text tokens only
      const int n0 = n_start + 1;
      const int nt = ntok[b] - n0 - 1;
      if (p >= n0 - 1 && p < n0 - 1 + nt) target[(size_t)p * B + b] = seq[b][p + 1];
    }
  }
  FW_HIP_AS(setup_fail, hipMemcpyAsync(heads_dev, sel_heads.data(), n_sel * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemcpyAsync(ntok_dev, ntok.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemcpyAsync(nfr_dev, nfr.data(), B * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemcpyAsync(g->prompt_dev, ptok.data(), ptok.size() * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemcpyAsync(target_dev, target.data(), target.size() * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemsetAsync(tprob, 0, (size_t)B * max_tok * sizeof(float), st));
  FW_HIP_AS(setup_fail, hipStreamSynchronize(st));
  // the text goes through the decoder in position blocks (a 100-token segment: 7 passes instead of 100); the selected
  // heads' cross-attention probabilities of every position, and the probability of the next text token where there is one
  auto targets_at = [&](int p) {
    for (int b = 0; b < B; ++b)
      if (target[(size_t)p * B + b] >= 0) return true;
    return false;
  };
  rc = pos_block_forward(
      m, lane, sc.gp, ptok, max_tok, B, max_tok, setup_fail,
      [&](StepCfg& s, int pos, int nb) {
        s.need_logits = false;
        for (int j = 0; j < nb; ++j) s.need_logits = s.need_logits || targets_at(pos + j);
        s.nospeech_rowmul = 0; s.done = g->zero_done;
        s.sel_heads_dev = heads_dev; s.sel_layer_off = layer_off.data(); s.probs = probs; s.n_sel_total = n_sel;
        s.kv_slot0 = kv_slot0;
        s.n_tok = max_tok; s.tok_idx = pos;
      },
      [&](int pos, int nb) {
        for (int j = 0; j < nb; ++j)
          if (targets_at(pos + j))
            fwd::launch_token_prob(st, g->logits + (size_t)j * c.n_vocab, c.n_vocab, target_dev + (size_t)(pos + j) * B, tprob,
                                   max_tok, pos + j, B, nb);
      });
  if (rc) return rc;
  launch_align_post(st, probs, stats, n_sel, max_tok, T, B, ntok_dev, nfr_dev, median_filter_width, mat);
  std::vector<float> hmat((size_t)B * max_tok * T), htprob((size_t)B * max_tok);
  FW_HIP_AS(run_fail, hipMemcpyAsync(hmat.data(), mat, hmat.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  FW_HIP_AS(run_fail, hipMemcpyAsync(htprob.data(), tprob, htprob.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  FW_HIP_AS(run_fail, hipStreamSynchronize(st));
  FW_HIP_AS(run_fail, hipGetLastError());
  prof_collect(lane->prof);
  const int n0 = n_start + 1;
  for (int b = 0; b < B; ++b) {
    const int nt = ntok[b] - n0 - 1;
    out_n_pairs[b] = 0;
    for (int i = 0; i < nt; ++i) out_probs[text_offsets[b] + i] = htprob[(size_t)b * max_tok + (n0 - 1 + i)];
    if (nt < 0) continue;
    // rows of the cost matrix: positions n_start .. n_start + nt (the <|notimestamps|> position, whose
    // attention predicts the first text token, up to the last text token; the <|endoftext|> row is dropped)
    // = nt + 1 rows, like openai-whisper's matrix[len(sot_sequence):-1].  The reference indexes the path's
    // token jumps with word boundaries up to nt (transcribe.py:1741-1745), so it needs exactly these rows.
    std::vector<int> ti, fi;
    fw::dtw_path(&hmat[((size_t)b * max_tok + n_start) * T], T, nt + 1, nfr[b], ti, fi);
    const int np = std::min((int)ti.size(), max_pairs);
    for (int i = 0; i < np; ++i) {
      out_pairs[((size_t)b * max_pairs + i) * 2] = ti[i];
      out_pairs[((size_t)b * max_pairs + i) * 2 + 1] = fi[i];
    }
    out_n_pairs[b] = np;
  }
  return FW_OK;
}

// ------------------------------------------------------------------------------------
// score: teacher-forced log-probs of GIVEN transcripts.  B chunks x H candidate sequences; sequence i = b * H + h is a
// decode chunk of its own (one cache slot, beam slot 0) that reads the cross-attention K / V^T of encoder chunk b, the way
// the hypotheses of a sampling run share theirs (kv_div = H).  prompt + targets go through the decoder in position
// blocks; a block that holds a target position gets its logits and ONE dec_score_kernel launch over all its rows.
// The logits at position P - 1 + k predict target k; position P - 1 + n_i predicts the <eot> that closes sequence i.
// ------------------------------------------------------------------------------------
extern "C" int32_t fw_score(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                            const int32_t* targets, const int32_t* target_offsets, int32_t B, int32_t H,
                            const fw_gen_opts* rules, float* out_token_logprobs, int32_t* out_best_ids,
                            float* out_best_logprobs) {
  return fw_score_boost(fm, enc_t, prompts, prompt_offsets, targets, target_offsets, B, H, rules, nullptr, out_token_logprobs,
                        out_best_ids, out_best_logprobs);
}

// fw_score with a boost list: fw_score_constrain without a constraint list
extern "C" int32_t fw_score_boost(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts, const int32_t* prompt_offsets,
                                  const int32_t* targets, const int32_t* target_offsets, int32_t B, int32_t H,
                                  const fw_gen_opts* rules, const fw_boost* boost, float* out_token_logprobs,
                                  int32_t* out_best_ids, float* out_best_logprobs) {
  return fw_score_constrain(fm, enc_t, prompts, prompt_offsets, targets, target_offsets, B, H, rules, boost, nullptr,
                            out_token_logprobs, out_best_ids, out_best_logprobs);
}

// fw_score with a boost list and / or a constraint list: dec_boost_kernel, then dec_constrain_kernel, on the block's logits
// (recomputed per block) in front of the scoring kernel
extern "C" int32_t fw_score_constrain(fw_model* fm, const fw_tensor* enc_t, const int32_t* prompts,
                                      const int32_t* prompt_offsets, const int32_t* targets, const int32_t* target_offsets,
                                      int32_t B, int32_t H, const fw_gen_opts* rules, const fw_boost* boost,
                                      const fw_constraint* constraint, float* out_token_logprobs, int32_t* out_best_ids,
                                      float* out_best_logprobs) {
  FW_CHECK_ARG(fm && enc_t && prompts && prompt_offsets && targets && target_offsets && out_token_logprobs, "null argument");
  FW_CHECK_ARG(!boost || rules, "a boost list needs rules: the boost is the first step of the decoding rules");
  FW_CHECK_ARG(!constraint || rules, "a constraint list needs rules: the constraint is a step of the decoding rules");
  FW_CHECK_ARG((out_best_ids == nullptr) == (out_best_logprobs == nullptr), "out_best_ids and out_best_logprobs go together");
  Model* m = decoder_of(&fm->impl);
  const Tensor* enc = &enc_t->impl;
  const fw_config& c = m->cfg;
  FW_CHECK_ARG(decoder_of(*enc) == m, "encoder output belongs to a different model");
  FW_CHECK_ARG(B == enc->B, "batch %d does not match the encoder output batch %d", B, enc->B);
  FW_CHECK_ARG(B >= 1 && B <= m->max_batch, "batch %d exceeds max_batch %d", B, m->max_batch);
  FW_CHECK_ARG(!boost || boost->n_vocab == c.n_vocab, "the boost list was built for a vocabulary of %d ids, the model has %d",
               boost ? boost->n_vocab : 0, c.n_vocab);
  if (constraint)
    if (int crc = constraint_check(constraint, c, rules, false)) return crc;
  if (!fwd::phrase_list_live(boost)) boost = nullptr;   // (an empty list does nothing)
  if (!fwd::phrase_list_live(constraint)) constraint = nullptr;
  FW_CHECK_ARG(H >= 1 && H <= m->max_beam, "%d candidates per chunk not in [1, max_beam=%d]", H, m->max_beam);
  FW_CHECK_ARG(c.n_vocab <= LP_SUP_WORDS * 64 && c.n_text_ctx <= 1024, "model too large for the scoring kernel");
  const int Bx = B * H;
  const int P = prompt_offsets[1] - prompt_offsets[0];
  FW_CHECK_ARG(P >= 1, "prompts must not be empty");
  int with_ts = 1;
  for (int b = 0; b < B; ++b) {
    FW_CHECK_ARG(prompt_offsets[b + 1] - prompt_offsets[b] == P,
                 "all prompts of a score() call must have the same length (prompt %d has %d tokens, expected %d)", b,
                 prompt_offsets[b + 1] - prompt_offsets[b], P);
    int wt = 1;
    for (int i = 0; i < P; ++i) {
      const int t = prompts[prompt_offsets[b] + i];
      FW_CHECK_ARG(t >= 0 && t < c.n_vocab, "prompt token %d out of range", t);
      if (t == c.tok_no_timestamps) wt = 0;
    }
    if (b == 0) with_ts = wt;
    FW_CHECK_ARG(!rules || wt == with_ts, "the prompts of a score() call with rules must agree on <|notimestamps|>");
  }
  FW_CHECK_ARG(target_offsets[0] >= 0, "bad target offsets");
  int max_n = 0;
  for (int i = 0; i < Bx; ++i) {
    const int n = target_offsets[i + 1] - target_offsets[i];
    FW_CHECK_ARG(n >= 0, "target offsets must not decrease (sequence %d)", i);
    FW_CHECK_ARG(P + n + 1 <= c.n_text_ctx, "prompt of %d + %d targets + <eot> exceed the text context %d (sequence %d)", P, n,
                 c.n_text_ctx, i);
    for (int k = 0; k < n; ++k) {
      const int t = targets[target_offsets[i] + k];
      FW_CHECK_ARG(t >= 0 && t < c.n_vocab, "target token %d out of range (sequence %d)", t, i);
    }
    max_n = std::max(max_n, n);
  }
  const int off0 = target_offsets[0];
  const size_t n_tgt = (size_t)(target_offsets[Bx] - off0), n_out = n_tgt + Bx;
  const int n_pos = P + max_n;                                   // positions 0 .. P - 1 + max_n
  const int ctx = std::min(c.n_text_ctx, (n_pos + 7) / 8 * 8);

  DecodeLane* lane = m->lanes[0].get();
  std::lock_guard<std::mutex> lk(lane->mu);
  int rc;
  const HipFail setup_fail{FW_ERUNTIME, "score setup"}, run_fail{FW_ERUNTIME, "score"};
  FW_HIP_AS(setup_fail, hipSetDevice(m->device));
  if ((rc = gen_workspace_ensure(m, lane))) return rc;
  GenWorkspace* g = lane->gen;
  FW_CHECK_ARG(Bx <= g->R && (int64_t)Bx * ctx <= g->self_cap,
               "this call needs %d decoder rows x %d positions; a lane of this model holds %d rows and %lld row-positions", Bx,
               ctx, g->R, (long long)g->self_cap);
  SingleCall sc;
  if ((rc = single_call_begin(m, lane, enc, n_pos, ctx, setup_fail, sc))) return rc;
  hipStream_t st = lane->stream;
  GenDev& gp = sc.gp;
  // one decode chunk per sequence, one cache slot each; H of them per encoder chunk (g->slot_map holds the B pool slots)
  gp.B = Bx; gp.K = 1; gp.kv_div = H; gp.cache_rows = Bx;
  fwd::fill_rule_fields(gp, c, rules, with_ts);
  gp.min_new = 0;   // a given token is scored, none is generated: min_new_tokens is not a rule of scoring (include/fwamd.h)

  std::vector<int> ptok((size_t)n_pos * Bx);
  std::vector<fwd::ScoreRow> tab((size_t)Bx * n_pos, fwd::ScoreRow{-1, 0, 0, 0});
  for (int i = 0; i < Bx; ++i) {
    const int32_t* pr = prompts + prompt_offsets[i / H];
    const int32_t* tg = targets + target_offsets[i];
    const int n = target_offsets[i + 1] - target_offsets[i];
    const int hist_off = target_offsets[i] - off0;
    for (int p = 0; p < n_pos; ++p) {
      ptok[(size_t)p * Bx + i] = p < P ? pr[p] : (p - P < n ? tg[p - P] : c.tok_eot);   // (padding rides along on <eot>)
      const int k = p - (P - 1);
      if (k >= 0 && k <= n) tab[(size_t)i * n_pos + p] = {k < n ? tg[k] : c.tok_eot, k, hist_off, hist_off + i + k};
    }
  }
  DevBufs tmp;   // (after `sc`: freed before the pool block is released)
  fwd::ScoreRow* tab_dev = nullptr;
  int *hist_dev = nullptr, *bid_dev = nullptr;
  float *lp_dev = nullptr, *blp_dev = nullptr;
  if ((rc = tmp.alloc(&tab_dev, tab.size())) || (rc = tmp.alloc(&hist_dev, std::max<size_t>(1, n_tgt))) ||
      (rc = tmp.alloc(&lp_dev, n_out)))
    return rc;
  if (out_best_ids && ((rc = tmp.alloc(&bid_dev, n_out)) || (rc = tmp.alloc(&blp_dev, n_out)))) return rc;
  int *boost_dev = nullptr, *constrain_dev = nullptr;
  const std::pair<const fw_phrase_table*, int**> lists[] = {{boost, &boost_dev}, {constraint, &constrain_dev}};
  for (const auto& [list, dev] : lists) {   // (null: no list of that kind, its pre-pass is not launched)
    if (!list) continue;
    if ((rc = tmp.alloc(dev, list->table.size()))) return rc;
    FW_HIP_AS(setup_fail, hipMemcpyAsync(*dev, list->table.data(), list->table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  FW_HIP_AS(setup_fail, hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(tab[0]), hipMemcpyHostToDevice, st));
  if (n_tgt) FW_HIP_AS(setup_fail, hipMemcpyAsync(hist_dev, targets + off0, n_tgt * sizeof(int), hipMemcpyHostToDevice, st));
  FW_HIP_AS(setup_fail, hipMemcpyAsync(g->prompt_dev, ptok.data(), ptok.size() * sizeof(int), hipMemcpyHostToDevice, st));
  std::vector<unsigned long long> mask;   // (lives until the synchronize below)
  if (rules) {
    mask = fwd::suppress_mask(rules->suppress_tokens, rules->n_suppress_tokens, c.n_vocab);
    FW_HIP_AS(setup_fail, hipMemcpyAsync(g->sup_bits, mask.data(), mask.size() * sizeof(mask[0]), hipMemcpyHostToDevice, st));
  }
  FW_HIP_AS(setup_fail, hipStreamSynchronize(st));
  rc = pos_block_forward(
      m, lane, gp, ptok, n_pos, Bx, n_pos, setup_fail,
      [&](StepCfg& s, int pos, int nb) {
        s.need_logits = pos + nb - 1 >= P - 1;   // every sequence has a target from position P - 1 on (its <eot> at least)
        s.nospeech_rowmul = 0; s.done = g->zero_done;
      },
      [&](int pos, int nb) {
        if (pos + nb - 1 < P - 1) return;
        ProfScope ps(lane->prof, PF_DEC_MISC, 0, 4.0 * Bx * nb * (double)c.n_vocab, st);
        if (boost_dev) fwd::launch_boost_score(st, gp, g->logits, boost_dev, tab_dev, n_pos, pos, nb, Bx * nb, hist_dev);
        if (constrain_dev)
          fwd::launch_constrain_score(st, gp, g->logits, constrain_dev, tab_dev, n_pos, pos, nb, Bx * nb, hist_dev);
        fwd::launch_score(st, gp, rules != nullptr, g->logits, g->sup_bits, tab_dev, n_pos, pos, nb, Bx * nb, hist_dev, lp_dev,
                          bid_dev, blp_dev);
      });
  if (rc) return rc;
  float* out_lp = out_token_logprobs + off0;
  FW_HIP_AS(run_fail, hipMemcpyAsync(out_lp, lp_dev, n_out * sizeof(float), hipMemcpyDeviceToHost, st));
  if (out_best_ids) {
    FW_HIP_AS(run_fail, hipMemcpyAsync(out_best_ids + off0, bid_dev, n_out * sizeof(int), hipMemcpyDeviceToHost, st));
    FW_HIP_AS(run_fail, hipMemcpyAsync(out_best_logprobs + off0, blp_dev, n_out * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  FW_HIP_AS(run_fail, hipStreamSynchronize(st));
  FW_HIP_AS(run_fail, hipGetLastError());
  prof_collect(lane->prof);
  return FW_OK;
}
