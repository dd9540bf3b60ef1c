// Silero VAD v6 on the GPU (MI355X-first form of csrc/vad_host.cpp).
//
// Validated on hardware against oracle/silero.py and the host path since round 4 (tests/test_gpu_vad.py, tests/test_gpu_c5.py);
// SileroVADModel(device="cuda") selects it.
//
// Two kernels (one hour of audio = 112 500 windows):
//   vad_front_kernel   one workgroup per 512-sample window: reflect pad, STFT as a [258 x 256] matrix product
//                      over 4 frames, magnitude, the four k=3 convolutions, the LSTM input projection
//                      gx = W feat + Wb + Rb.  Window-parallel: 112 500 workgroups, the 1.2 MB of weights stay
//                      in L2; all reduction loops run in the order of the definition (k outer, channel inner).
//   vad_lstm_kernel    ONE workgroup of 512 threads walks the windows sequentially: thread r keeps row r of the
//                      recurrence matrix R[512][128] in 128 VGPRs, h[128] lives in LDS (broadcast reads), two
//                      barriers per step; c stays in the registers of the first 128 threads.
//
// N recordings in one call (fw_vad_forward_audio_batch_dev): the same two bodies (vad_front_body, vad_lstm_body — the
// arithmetic exists once) behind two ragged kernels.  vad_front_ragged_kernel is one launch over the windows of a group of
// recordings, a workgroup finds its recording in a device table of first windows and frames within it;
// vad_lstm_ragged_kernel is one workgroup PER RECORDING, all launched together: the recurrence is a latency chain of one
// workgroup on one CU, so N recordings cost about the time of the longest one (more recordings than CUs queue behind).
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "engine.h"
#include "vad_model.h"

namespace {

struct VadDev {
  int device = 0;
  hipStream_t st = nullptr;
  float *basis_t = nullptr, *cw_t[4] = {nullptr, nullptr, nullptr, nullptr}, *cb[4] = {nullptr, nullptr, nullptr, nullptr};
  float *lw_t = nullptr, *lr_t = nullptr, *lb = nullptr, *dw = nullptr;
  float db = 0.f;
};

__device__ __forceinline__ float sigmoid_dev(float x) { return 1.0f / (1.0f + __expf(-x)); }

// one window of one recording: wi = its index in the recording, n_windows = the recording's windows, audio = the recording's
// first sample (or win: the framed rows), gx_row = where the window's 512 gate pre-activations go
__device__ __forceinline__ void vad_front_body(const float* __restrict__ win, const float* __restrict__ basis_t,
                                               const float* __restrict__ cw0, const float* __restrict__ cb0,
                                               const float* __restrict__ cw1, const float* __restrict__ cb1,
                                               const float* __restrict__ cw2, const float* __restrict__ cb2,
                                               const float* __restrict__ cw3, const float* __restrict__ cb3,
                                               const float* __restrict__ lw_t, const float* __restrict__ lb,
                                               float* __restrict__ gx_row, const float* __restrict__ audio,
                                               const int64_t wi, const int64_t n_windows) {
  __shared__ float xp[kPadded];
  __shared__ float spec[kFrames][2 * kBins];
  __shared__ float mag[kFrames][kBins + 3];
  __shared__ float a0[4][128];
  __shared__ float a1[2][64];
  __shared__ float a2[64];
  __shared__ float feat[128];
  const int tid = threadIdx.x;
  // sample j of this window.  win: the caller framed [context 64 | window 512] rows.  audio (round 6): framed HERE, as the
  // reference's SileroVADModel.__call__ does on the host (vad.py:318-336): the context of window i is the tail of window
  // i - 1 (zeros for the first window) and the last 64 samples of the LAST window are zeroed (its in-place
  // `context[-1] = 0` on a view) — no [n][576] copy of the recording is built on the host or sent over PCIe
  const float* w = win ? win + (size_t)wi * kWin : nullptr;
  auto sample = [&](int j) -> float {
    if (w) return w[j];
    if (j < 64) return wi == 0 ? 0.f : audio[(wi - 1) * 512 + 448 + j];
    const int jj = j - 64;
    if (wi == n_windows - 1 && jj >= 448) return 0.f;
    return audio[wi * 512 + jj];
  };
  for (int i = tid; i < kWin; i += 256) xp[kPad + i] = sample(i);
  if (tid < kPad) {
    xp[tid] = sample(kPad - tid);                // reflect, edge sample not repeated
    xp[kPad + kWin + tid] = sample(kWin - 2 - tid);
  }
  __syncthreads();
  // STFT: frames 1..4 of the stride-128 convolution (frame 0 is sliced away by the graph)
  for (int k = tid; k < 2 * kBins; k += 256) {
    float acc[kFrames] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < kTaps; ++i) {
      const float b = basis_t[(size_t)i * 2 * kBins + k];
#pragma unroll
      for (int t = 0; t < kFrames; ++t) acc[t] += b * xp[(t + 1) * kHop + i];
    }
#pragma unroll
    for (int t = 0; t < kFrames; ++t) spec[t][k] = acc[t];
  }
  __syncthreads();
  for (int idx = tid; idx < kFrames * kBins; idx += 256) {
    const int t = idx / kBins, c = idx - t * kBins;
    const float re = spec[t][c], im = spec[t][c + kBins];
    mag[t][c] = sqrtf(re * re + im * im);
  }
  __syncthreads();
  {  // conv 129 -> 128, stride 1: thread = (output channel, frame pair)
    const int o = tid & 127, tp = tid >> 7;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int t = 2 * tp + tt;
      float acc = cb0[o];
      for (int k = 0; k < 3; ++k) {
        const int ti = t + k - 1;
        if (ti < 0 || ti >= 4) continue;
        for (int c = 0; c < kBins; ++c) acc += cw0[((size_t)c * 3 + k) * 128 + o] * mag[ti][c];
      }
      a0[t][o] = acc > 0.f ? acc : 0.f;
    }
  }
  __syncthreads();
  if (tid < 128) {  // conv 128 -> 64, stride 2: 2 output frames
    const int o = tid & 63, t = tid >> 6;
    float acc = cb1[o];
    for (int k = 0; k < 3; ++k) {
      const int ti = 2 * t + k - 1;
      if (ti < 0 || ti >= 4) continue;
      for (int c = 0; c < 128; ++c) acc += cw1[((size_t)c * 3 + k) * 64 + o] * a0[ti][c];
    }
    a1[t][o] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  if (tid < 64) {   // conv 64 -> 64, stride 2: 1 output frame
    float acc = cb2[tid];
    for (int k = 0; k < 3; ++k) {
      const int ti = k - 1;
      if (ti < 0 || ti >= 2) continue;
      for (int c = 0; c < 64; ++c) acc += cw2[((size_t)c * 3 + k) * 64 + tid] * a1[ti][c];
    }
    a2[tid] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  if (tid < 128) {  // conv 64 -> 128 on one frame: only the centre tap meets data
    float acc = cb3[tid];
    for (int c = 0; c < 64; ++c) acc += cw3[((size_t)c * 3 + 1) * 128 + tid] * a2[c];
    feat[tid] = acc > 0.f ? acc : 0.f;
  }
  __syncthreads();
  for (int g = tid; g < kGates; g += 256) {
    float acc = lb[g];
    for (int c = 0; c < kHidden; ++c) acc += lw_t[(size_t)c * kGates + g] * feat[c];
    gx_row[g] = acc;
  }
}

#define VAD_FRONT_WEIGHT_PARAMS                                                                                          \
  const float *__restrict__ basis_t, const float *__restrict__ cw0, const float *__restrict__ cb0,                       \
      const float *__restrict__ cw1, const float *__restrict__ cb1, const float *__restrict__ cw2,                       \
      const float *__restrict__ cb2, const float *__restrict__ cw3, const float *__restrict__ cb3,                       \
      const float *__restrict__ lw_t, const float *__restrict__ lb
#define VAD_FRONT_WEIGHT_ARGS basis_t, cw0, cb0, cw1, cb1, cw2, cb2, cw3, cb3, lw_t, lb

__global__ __launch_bounds__(256) void vad_front_kernel(const float* __restrict__ win, VAD_FRONT_WEIGHT_PARAMS,
                                                        float* __restrict__ gx, const float* __restrict__ audio,
                                                        int64_t n_windows) {
  vad_front_body(win, VAD_FRONT_WEIGHT_ARGS, gx + (size_t)blockIdx.x * kGates, audio, blockIdx.x, n_windows);
}

// A group of recordings, one workgroup per window of the group.  first_win[0 .. n_rec]: first window of every recording of
// the group (non-decreasing; first_win[n_rec] = the end), audio / gx: the group's first sample / first gate row.  The grid
// is first_win[n_rec] - first_win[0] workgroups, so every workgroup's window lies in exactly one non-empty recording:
// the one with first_win[r] <= window < first_win[r + 1] (an empty recording has no such window and is never picked).
__global__ __launch_bounds__(256) void vad_front_ragged_kernel(VAD_FRONT_WEIGHT_PARAMS, float* __restrict__ gx,
                                                               const float* __restrict__ audio,
                                                               const int64_t* __restrict__ first_win, int n_rec) {
  const int64_t base = first_win[0], g = base + blockIdx.x;
  int lo = 0, hi = n_rec;                        // first_win[lo] <= g < first_win[hi] throughout
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first_win[mid] <= g) lo = mid; else hi = mid;
  }
  const int64_t first = first_win[lo];
  vad_front_body(nullptr, VAD_FRONT_WEIGHT_ARGS, gx + (size_t)blockIdx.x * kGates, audio + (first - base) * 512, g - first,
                 first_win[lo + 1] - first);
}

// the recurrence over the n windows of ONE recording, by one workgroup of 512 threads
__device__ __forceinline__ void vad_lstm_body(const float* __restrict__ gx, const float* __restrict__ lr_t,
                                              const float* __restrict__ dw, float db, int64_t n,
                                              float* __restrict__ h_io, float* __restrict__ c_io,
                                              float* __restrict__ probs) {
  __shared__ float hs[kHidden];
  __shared__ float gs[kGates];
  __shared__ float part[2];
  const int r = threadIdx.x;
  float R[kHidden];
#pragma unroll
  for (int k = 0; k < kHidden; ++k) R[k] = lr_t[(size_t)k * kGates + r];   // row r of the recurrence matrix
  float cell = 0.f;
  if (r < kHidden) {
    hs[r] = h_io[r];
    cell = c_io[r];
  }
  const float dwr = r < kHidden ? dw[r] : 0.f;
  __syncthreads();
  float g_next = n > 0 ? gx[r] : 0.f;
  for (int64_t i = 0; i < n; ++i) {
    float g = g_next;
    if (i + 1 < n) g_next = gx[(size_t)(i + 1) * kGates + r];           // in flight during the dot product
    // four interleaved partial sums (k = 0, 4, 8, ... / 1, 5, ... / ...): the step is a chain of DEPENDENT fused
    // multiply-adds — 128 in a row were ~0.45 us of the ~1.1 us a step took, and an 8 h recording is 900 000 steps in front
    // of the first transcribed chunk (profiles/r06_vad_bench.json); the order of the additions differs from the host path's
    // k-ascending sum by fp32 round-off only (tests/test_gpu_vad.py: 1e-4 / 5e-5 bounds, measured ~1e-7)
    float g1 = 0.f, g2 = 0.f, g3 = 0.f;
#pragma unroll
    for (int k = 0; k < kHidden; k += 4) {                               // LDS broadcast reads
      g += R[k] * hs[k];
      g1 += R[k + 1] * hs[k + 1];
      g2 += R[k + 2] * hs[k + 2];
      g3 += R[k + 3] * hs[k + 3];
    }
    g = (g + g1) + (g2 + g3);
    gs[r] = g;
    __syncthreads();
    if (r < kHidden) {   // ONNX gate order i, o, f, c
      const float ig = sigmoid_dev(gs[r]), og = sigmoid_dev(gs[kHidden + r]), fg = sigmoid_dev(gs[2 * kHidden + r]);
      cell = fg * cell + ig * tanhf(gs[3 * kHidden + r]);
      const float hn = og * tanhf(cell);
      hs[r] = hn;
      float y = hn > 0.f ? dwr * hn : 0.f;
      y = wave_sum(y);
      if ((r & 63) == 0) part[r >> 6] = y;
    }
    __syncthreads();
    if (r == 0) probs[i] = sigmoid_dev(db + part[0] + part[1]);
  }
  if (r < kHidden) {
    h_io[r] = hs[r];
    c_io[r] = cell;
  }
}

__global__ __launch_bounds__(512) void vad_lstm_kernel(const float* __restrict__ gx, const float* __restrict__ lr_t,
                                                       const float* __restrict__ dw, float db, int64_t n,
                                                       float* __restrict__ h_io, float* __restrict__ c_io,
                                                       float* __restrict__ probs) {
  vad_lstm_body(gx, lr_t, dw, db, n, h_io, c_io, probs);
}

// one workgroup per recording of a group (first_win as above; gx / probs: the group's first row / value; h_io, c_io:
// [n_rec][128]).  A recording of no windows leaves its state as it is.
__global__ __launch_bounds__(512) void vad_lstm_ragged_kernel(const float* __restrict__ gx, const float* __restrict__ lr_t,
                                                              const float* __restrict__ dw, float db,
                                                              const int64_t* __restrict__ first_win,
                                                              float* __restrict__ h_io, float* __restrict__ c_io,
                                                              float* __restrict__ probs) {
  const int64_t first = first_win[blockIdx.x], n = first_win[blockIdx.x + 1] - first, at = first - first_win[0];
  if (n == 0) return;
  vad_lstm_body(gx + (size_t)at * kGates, lr_t, dw, db, n, h_io + (size_t)blockIdx.x * kHidden,
                c_io + (size_t)blockIdx.x * kHidden, probs + at);
}

// (Round 6 measured a second form — four waves, two gate rows per lane, the four gates of a unit meeting by one cross-lane
//  exchange, h double-buffered so that a step has ONE barrier — at 2.30 s for the 900 000 windows of an 8 h recording against
//  1.79 s for the form above: 256 registers of recurrence matrix per lane and half the waves to hide the LDS broadcast reads.
//  Removed; profiles/r06_vad_bench_call9_lstm_forms.json.)
template <typename T>
int upload(const std::vector<T>& src, T** dst) {
  FW_HIP(hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(T)));
  FW_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return FW_OK;
}

int ensure_dev(fw_vad* v, int device) {
  if (v->dev) {
    if (static_cast<VadDev*>(v->dev)->device == device) return FW_OK;
    fw_vad_dev_release(v->dev);
    v->dev = nullptr;
  }
  FW_HIP(hipSetDevice(device));
  VadDev* d = new VadDev();
  d->device = device;
  v->dev = d;   // released by fw_vad_free even if an upload below fails
  const Vad& m = v->impl;
  int rc;
  if ((rc = upload(m.basis_t, &d->basis_t))) return rc;
  for (int i = 0; i < 4; ++i) {
    if ((rc = upload(m.cw_t[i], &d->cw_t[i]))) return rc;
    if ((rc = upload(m.cb[i], &d->cb[i]))) return rc;
  }
  if ((rc = upload(m.lw_t, &d->lw_t))) return rc;
  if ((rc = upload(m.lr_t, &d->lr_t))) return rc;
  if ((rc = upload(m.lb, &d->lb))) return rc;
  if ((rc = upload(m.dw, &d->dw))) return rc;
  d->db = m.db;
  FW_HIP(hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking));
  return FW_OK;
}

}  // namespace

void fw_vad_dev_release(void* dev) {
  VadDev* d = static_cast<VadDev*>(dev);
  if (!d) return;
  (void)hipSetDevice(d->device);
  float* ptrs[] = {d->basis_t, d->cw_t[0], d->cw_t[1], d->cw_t[2], d->cw_t[3], d->cb[0], d->cb[1], d->cb[2], d->cb[3],
                   d->lw_t,    d->lr_t,    d->lb,      d->dw};
  for (float* p : ptrs)
    if (p) (void)hipFree(p);
  if (d->st) (void)hipStreamDestroy(d->st);
  delete d;
}

// windows != null: n framed rows of 576 samples; audio != null: n * 512 samples, framed on the device
static int32_t vad_forward_dev_impl(fw_vad* v, int32_t device_index, const float* windows, const float* audio, int64_t n,
                                    float* h, float* c, float* probs) {
  FW_CHECK_ARG(v && h && c && (n == 0 || ((windows || audio) && probs)), "null argument");
  FW_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "window count out of range");
  if (n == 0) return FW_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_index < 0 || device_index >= ndev) {
    fw::set_error("fw_vad_forward_dev: no HIP device %d", device_index);
    return FW_ENODEV;
  }
  int rc = ensure_dev(v, device_index);
  if (rc) return rc;
  VadDev* d = static_cast<VadDev*>(v->dev);
  FW_HIP(hipSetDevice(d->device));
  float *dwin = nullptr, *dgx = nullptr, *dh = nullptr, *dc = nullptr, *dp = nullptr;
  auto cleanup = [&]() {
    for (float* p : {dwin, dgx, dh, dc, dp})
      if (p) (void)hipFree(p);
  };
#define VAD_TRY(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fw::set_error("%s failed: %s", #call, hipGetErrorString(e_));                          \
      cleanup();                                                                             \
      return e_ == hipErrorOutOfMemory ? FW_ENOMEM : FW_ERUNTIME;                            \
    }                                                                                        \
  } while (0)
  const size_t in_floats = windows ? (size_t)n * kWin : (size_t)n * 512;
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dwin), in_floats * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dgx), (size_t)n * kGates * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dh), kHidden * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dc), kHidden * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dp), (size_t)n * sizeof(float)));
  VAD_TRY(hipMemcpyAsync(dwin, windows ? windows : audio, in_floats * sizeof(float), hipMemcpyHostToDevice, d->st));
  VAD_TRY(hipMemcpyAsync(dh, h, kHidden * sizeof(float), hipMemcpyHostToDevice, d->st));
  VAD_TRY(hipMemcpyAsync(dc, c, kHidden * sizeof(float), hipMemcpyHostToDevice, d->st));
  vad_front_kernel<<<(unsigned)n, 256, 0, d->st>>>(windows ? dwin : nullptr, d->basis_t, d->cw_t[0], d->cb[0], d->cw_t[1],
                                                   d->cb[1], d->cw_t[2], d->cb[2], d->cw_t[3], d->cb[3], d->lw_t, d->lb, dgx,
                                                   windows ? nullptr : dwin, n);
  vad_lstm_kernel<<<1, 512, 0, d->st>>>(dgx, d->lr_t, d->dw, d->db, n, dh, dc, dp);
  VAD_TRY(hipGetLastError());
  VAD_TRY(hipMemcpyAsync(probs, dp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipMemcpyAsync(h, dh, kHidden * sizeof(float), hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipMemcpyAsync(c, dc, kHidden * sizeof(float), hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipStreamSynchronize(d->st));
#undef VAD_TRY
  cleanup();
  return FW_OK;
}

extern "C" int32_t fw_vad_forward_dev(fw_vad* v, int32_t device_index, const float* windows, int64_t n, float* h,
                                      float* c, float* probs) {
  return vad_forward_dev_impl(v, device_index, windows, nullptr, n, h, c, probs);
}

extern "C" int32_t fw_vad_forward_audio_dev(fw_vad* v, int32_t device_index, const float* audio, int64_t n_samples,
                                            float* h, float* c, float* probs) {
  FW_CHECK_ARG(n_samples >= 0 && n_samples % 512 == 0, "the recording must be padded to a multiple of 512 samples");
  return vad_forward_dev_impl(v, device_index, nullptr, audio, n_samples / 512, h, c, probs);
}

extern "C" int32_t fw_vad_forward_audio_batch_dev(fw_vad* v, int32_t device_index, const float* audio,
                                                  const int64_t* offsets, int32_t n_rec, float* h, float* c,
                                                  float* probs) {
  FW_CHECK_ARG(v && n_rec >= 0, "null model or negative recording count");
  if (n_rec == 0) return FW_OK;
  FW_CHECK_ARG(offsets && h && c, "null argument");
  FW_CHECK_ARG(offsets[0] >= 0 && offsets[0] % 512 == 0, "offsets must be non-negative multiples of 512 samples");
  std::vector<int64_t> first((size_t)n_rec + 1);           // first window of every recording, relative to offsets[0]
  first[0] = 0;
  for (int r = 0; r < n_rec; ++r) {
    FW_CHECK_ARG(offsets[r + 1] >= offsets[r], "offsets must not decrease (recording %d)", r);
    FW_CHECK_ARG(offsets[r + 1] % 512 == 0, "every recording must be padded to a multiple of 512 samples (recording %d)", r);
    FW_CHECK_ARG(offsets[r + 1] - offsets[r] < ((int64_t)512 << 31), "window count out of range (recording %d)", r);
    first[r + 1] = (offsets[r + 1] - offsets[0]) / 512;
  }
  const int64_t total = first[n_rec];
  if (total == 0) return FW_OK;
  FW_CHECK_ARG(audio && probs, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_index < 0 || device_index >= ndev) {
    fw::set_error("fw_vad_forward_audio_batch_dev: no HIP device %d", device_index);
    return FW_ENODEV;
  }
  // groups of consecutive recordings of at most FW_VAD_BATCH_MAX_WINDOWS windows (a longer recording: a group of its own)
  std::vector<int> cut{0};
  int64_t largest = 0;
  for (int r = 0; r < n_rec;) {
    int e = r + 1;
    while (e < n_rec && first[e + 1] - first[r] <= FW_VAD_BATCH_MAX_WINDOWS) ++e;
    largest = std::max(largest, first[e] - first[r]);
    cut.push_back(e);
    r = e;
  }
  int rc = ensure_dev(v, device_index);
  if (rc) return rc;
  VadDev* d = static_cast<VadDev*>(v->dev);
  FW_HIP(hipSetDevice(d->device));
  float *daudio = nullptr, *dgx = nullptr, *dh = nullptr, *dc = nullptr, *dp = nullptr;
  int64_t* dfirst = nullptr;
  auto cleanup = [&]() {
    for (void* p : {(void*)daudio, (void*)dgx, (void*)dh, (void*)dc, (void*)dp, (void*)dfirst})
      if (p) (void)hipFree(p);
  };
#define VAD_TRY(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fw::set_error("%s failed: %s", #call, hipGetErrorString(e_));                          \
      cleanup();                                                                             \
      return e_ == hipErrorOutOfMemory ? FW_ENOMEM : FW_ERUNTIME;                            \
    }                                                                                        \
  } while (0)
  const size_t state_bytes = (size_t)n_rec * kHidden * sizeof(float);
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&daudio), (size_t)largest * 512 * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dgx), (size_t)largest * kGates * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dh), state_bytes));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dc), state_bytes));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dp), (size_t)total * sizeof(float)));
  VAD_TRY(hipMalloc(reinterpret_cast<void**>(&dfirst), first.size() * sizeof(int64_t)));
  VAD_TRY(hipMemcpyAsync(dfirst, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice, d->st));
  VAD_TRY(hipMemcpyAsync(dh, h, state_bytes, hipMemcpyHostToDevice, d->st));
  VAD_TRY(hipMemcpyAsync(dc, c, state_bytes, hipMemcpyHostToDevice, d->st));
  for (size_t g = 0; g + 1 < cut.size(); ++g) {
    const int r0 = cut[g], nr = cut[g + 1] - r0;
    const int64_t w0 = first[r0], nw = first[r0 + nr] - w0;
    if (nw == 0) continue;
    // (the stream orders this upload behind the kernels of the group before, which read the same buffer)
    VAD_TRY(hipMemcpyAsync(daudio, audio + offsets[0] + w0 * 512, (size_t)nw * 512 * sizeof(float), hipMemcpyHostToDevice,
                           d->st));
    vad_front_ragged_kernel<<<(unsigned)nw, 256, 0, d->st>>>(d->basis_t, d->cw_t[0], d->cb[0], d->cw_t[1], d->cb[1],
                                                             d->cw_t[2], d->cb[2], d->cw_t[3], d->cb[3], d->lw_t, d->lb,
                                                             dgx, daudio, dfirst + r0, nr);
    vad_lstm_ragged_kernel<<<(unsigned)nr, 512, 0, d->st>>>(dgx, d->lr_t, d->dw, d->db, dfirst + r0,
                                                            dh + (size_t)r0 * kHidden, dc + (size_t)r0 * kHidden, dp + w0);
    VAD_TRY(hipGetLastError());
  }
  VAD_TRY(hipMemcpyAsync(probs, dp, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipMemcpyAsync(h, dh, state_bytes, hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipMemcpyAsync(c, dc, state_bytes, hipMemcpyDeviceToHost, d->st));
  VAD_TRY(hipStreamSynchronize(d->st));
#undef VAD_TRY
  cleanup();
  return FW_OK;
}
