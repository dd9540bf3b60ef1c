// Sample-rate conversion of file audio on the GPU (device form of
// faster_whisper_amd/audio.py::resample): Kaiser-windowed-sinc polyphase FIR, float32 in, fp64 accumulate, float32 out.
//
// Definition (audio.py::resample): g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, big = max(up, down),
// half = taps_per_phase * big / 2, prototype h[t], t = -half .. half, = 2c sinc(2c t) kaiser(2 half + 1, beta)[t] with
// c = 0.5 / big, scaled to sum up;  y[m] = sum_k h[half + k up - m down] x[k] over |k up - m down| <= half, x zero outside
// [0, n).  Output m meets the taps j0, j0 + up, ... with j0 = (half - m down) mod up, which depends on m mod up only (the
// PHASE), and the inputs k0, k0 + 1, ... with k0 = (m down - half + j0) / up = ceil((m down - half) / up).
//
// resample_kernel   one workgroup per run of consecutive outputs (256, fewer when down / up is so large that their input
//                   span would not fit the LDS): the input span of the run is staged in LDS once (~800 floats for 256
//                   outputs at 441 / 160) and every thread walks its own phase's row of the coefficient table [up][taps]
//                   (fp64, 114 KB at 441 / 160: L2-resident); with a single phase (up == 1) the row is staged in LDS too.
//                   fp64 FMA chain in ascending k: the s16 waveform equals the host path's sample for sample.
// fw_resample_dev   the recording goes through in bounded blocks of outputs on two streams with a buffer pair each, so
//                   that block i + 1's upload runs under block i's kernel and download and device memory does not grow
//                   with the recording.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "../../include/fwamd_test.h"
#include "common.h"
#include "engine.h"

namespace {

constexpr int kThreads = 256;                       // threads, and at most outputs, per workgroup
constexpr int64_t kLdsBytes = 64 * 1024;            // dynamic LDS a workgroup may ask for
constexpr int64_t kMaxFilter = (int64_t)1 << 22;    // prototype taps (32 MB of fp64): 11 025 -> 16 000 Hz has 20 481
constexpr int64_t kDefaultBlock = (int64_t)1 << 20; // outputs per block: 4 MB down, 11.6 MB up at 441 / 160
constexpr int64_t kMaxBlock = (int64_t)1 << 28;

struct Filter {
  int up = 1, down = 1;
  int64_t half = 0;
  std::vector<double> h;   // [2 half + 1]
};

// what one call needs on the device besides the audio
struct Plan {
  int up = 1, down = 1, taps = 1;   // taps: of the longest phase = row length of `table`
  int64_t half = 0;
  std::vector<double> table;        // [up][taps]: row p = h[j0(p)], h[j0(p) + up], ..., zero-padded
  int outs_per_wg = kThreads;
  size_t lds_bytes = 0;
};

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// I0 by its power series sum_k ((x / 2)^2k / (k!)^2): all terms positive, so the sum is accurate to a few ulp
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

int design(int32_t rate_in, int32_t rate_out, int32_t taps_per_phase, double beta, Filter* f) {
  FW_CHECK_ARG(rate_in > 0 && rate_out > 0, "fw_resample: sample rates must be positive (got %d -> %d)", rate_in, rate_out);
  FW_CHECK_ARG(taps_per_phase >= 2, "fw_resample: taps_per_phase must be at least 2 (got %d)", taps_per_phase);
  FW_CHECK_ARG(beta >= 0.0 && beta <= 100.0, "fw_resample: Kaiser beta %g out of range", beta);
  const int64_t g = gcd64(rate_in, rate_out);
  f->up = (int)(rate_out / g);
  f->down = (int)(rate_in / g);
  const int64_t big = f->up > f->down ? f->up : f->down;
  f->half = (int64_t)taps_per_phase * big / 2;
  FW_CHECK_ARG(2 * f->half + 1 <= kMaxFilter, "fw_resample: %d -> %d Hz with %d taps per phase needs a prototype filter of "
               "%lld taps (limit %lld)", rate_in, rate_out, taps_per_phase, (long long)(2 * f->half + 1), (long long)kMaxFilter);
  return FW_OK;
}

void fill(Filter* f, double beta) {
  const int64_t half = f->half, n_h = 2 * half + 1;
  const double cutoff = 0.5 / (double)(f->up > f->down ? f->up : f->down), inv_i0 = bessel_i0(beta);
  f->h.resize((size_t)n_h);
  double sum = 0.0, comp = 0.0;                          // Neumaier-compensated sum of the taps
  for (int64_t i = 0; i < n_h; ++i) {
    const double t = (double)(i - half);
    const double sx = 2.0 * cutoff * t, y = M_PI * (sx == 0.0 ? 1e-20 : sx);
    const double r = t / (double)half;
    const double w = bessel_i0(beta * sqrt(1.0 - r * r)) / inv_i0;
    const double v = 2.0 * cutoff * (sin(y) / y) * w;
    f->h[(size_t)i] = v;
    const double s = sum + v;
    comp += fabs(sum) >= fabs(v) ? (sum - s) + v : (v - s) + sum;
    sum = s;
  }
  const double scale = (double)f->up / (sum + comp);
  for (double& v : f->h) v *= scale;
}

// LDS bytes of a workgroup of `outs` consecutive outputs: their input span, plus the coefficient row when there is one phase
int64_t lds_bytes_for(const Plan& p, int outs) {
  const int64_t span = ceil_div((int64_t)(outs - 1) * p.down, p.up) + p.taps + 1;
  return (p.up == 1 ? (int64_t)p.taps * 8 : 0) + span * 4;
}

int make_plan(const Filter& f, Plan* p) {
  p->up = f.up;
  p->down = f.down;
  p->half = f.half;
  const int64_t n_h = 2 * f.half + 1;
  p->taps = (int)ceil_div(n_h, f.up);
  p->table.assign((size_t)f.up * p->taps, 0.0);
  for (int ph = 0; ph < f.up; ++ph) {
    int64_t j0 = (f.half - (int64_t)ph * f.down) % f.up;
    if (j0 < 0) j0 += f.up;
    for (int64_t j = j0, i = 0; j < n_h; j += f.up, ++i) p->table[(size_t)ph * p->taps + i] = f.h[(size_t)j];
  }
  p->outs_per_wg = kThreads;
  while (p->outs_per_wg > 1 && lds_bytes_for(*p, p->outs_per_wg) > kLdsBytes) p->outs_per_wg /= 2;
  FW_CHECK_ARG(lds_bytes_for(*p, p->outs_per_wg) <= kLdsBytes, "fw_resample: one output of this conversion reads %d input "
               "samples, more than the device kernel stages", p->taps);
  p->lds_bytes = (size_t)lds_bytes_for(*p, p->outs_per_wg);
  return FW_OK;
}

// x: samples [k_lo, k_lo + n_x) of the recording (everything the launch's outputs meet inside [0, n)); out: outputs
// [m_lo, m_lo + n_m).  All positions on the zero-stuffed grid (m down, k up) are 64-bit: m down passes 2^31 after five
// minutes of 44.1 kHz audio.
template <bool kOnePhase>
__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ x, int64_t k_lo, int64_t n_x,
                                                            const double* __restrict__ table, int up, int down,
                                                            int64_t half, int taps, int64_t m_lo, int64_t n_m,
                                                            int outs_per_wg, int quantize_s16, float* __restrict__ out) {
  extern __shared__ double smem[];
  double* cs = smem;                                                        // [taps] when kOnePhase
  float* xs = reinterpret_cast<float*>(smem + (kOnePhase ? taps : 0));     // the workgroup's input span
  const int tid = threadIdx.x;
  const int64_t w_lo = (int64_t)blockIdx.x * outs_per_wg;                   // first output of the workgroup, within the launch
  const int n_w = (int)(n_m - w_lo < outs_per_wg ? n_m - w_lo : outs_per_wg);
  const int64_t k_first = ceil_div((m_lo + w_lo) * down - half, up);
  const int span = (int)(ceil_div((m_lo + w_lo + n_w - 1) * down - half, up) - k_first) + taps;
  for (int i = tid; i < span; i += kThreads) {
    const int64_t k = k_first + i - k_lo;
    xs[i] = k >= 0 && k < n_x ? x[k] : 0.f;
  }
  if (kOnePhase)
    for (int i = tid; i < taps; i += kThreads) cs[i] = table[i];
  __syncthreads();
  if (tid >= n_w) return;
  const int64_t c = (m_lo + w_lo + tid) * down;                             // this output on the zero-stuffed grid
  int j0 = (int)((half - c) % up);
  if (j0 < 0) j0 += up;
  const int64_t k0 = (c - half + j0) / up;                                  // exact
  const int n_taps = (int)((2 * half + 1 - j0 + up - 1) / up);              // of this phase (<= taps)
  const double* cf = kOnePhase ? cs : table + (size_t)((m_lo + w_lo + tid) % up) * taps;
  const float* xw = xs + (k0 - k_first);
  double acc = 0.0;
#pragma unroll 4
  for (int i = 0; i < n_taps; ++i) acc = fma(cf[i], (double)xw[i], acc);
  float y = (float)acc;
  if (quantize_s16) {   // audio.py::_to_s16_float on the float32 sample `resample` returns: clip(rint(y * 32768), -32768,
                        // 32767) / 32768 in fp64, rint = round half to even; every k / 32768 is a float32
    const double q = rint((double)y * 32768.0);
    y = (float)((q < -32768.0 ? -32768.0 : q > 32767.0 ? 32767.0 : q) / 32768.0);
  }
  out[w_lo + tid] = y;
}

void launch(const Plan& p, const double* table_dev, const float* x_dev, int64_t k_lo, int64_t n_x, int64_t m_lo, int64_t n_m,
            int quantize_s16, float* out_dev, hipStream_t st) {
  const unsigned grid = (unsigned)ceil_div(n_m, p.outs_per_wg);
  if (p.up == 1)
    resample_kernel<true><<<grid, kThreads, p.lds_bytes, st>>>(x_dev, k_lo, n_x, table_dev, p.up, p.down, p.half, p.taps, m_lo,
                                                                n_m, p.outs_per_wg, quantize_s16, out_dev);
  else
    resample_kernel<false><<<grid, kThreads, p.lds_bytes, st>>>(x_dev, k_lo, n_x, table_dev, p.up, p.down, p.half, p.taps,
                                                                 m_lo, n_m, p.outs_per_wg, quantize_s16, out_dev);
}

// input samples [*lo, *hi) of a recording of n samples that outputs [m_lo, m_lo + n_m) meet
void input_span(const Plan& p, int64_t n, int64_t m_lo, int64_t n_m, int64_t* lo, int64_t* hi) {
  const int64_t a = ceil_div(m_lo * p.down - p.half, p.up), b = ceil_div((m_lo + n_m - 1) * p.down - p.half, p.up) + p.taps;
  *lo = a < 0 ? 0 : (a > n ? n : a);
  *hi = b > n ? n : (b < *lo ? *lo : b);
}

// arguments of fw_resample_dev / fw_bench_resample -> plan
int plan_call(const float* x, int64_t n, int32_t rate_in, int32_t rate_out, int32_t taps_per_phase, double beta,
              const float* out, int64_t n_out, Plan* plan) {
  Filter f;
  int rc = design(rate_in, rate_out, taps_per_phase, beta, &f);
  if (rc) return rc;
  const int64_t big = f.up > f.down ? f.up : f.down;
  FW_CHECK_ARG(n >= 0 && n <= (INT64_MAX >> 2) / big, "fw_resample: sample count %lld out of range", (long long)n);
  FW_CHECK_ARG(n_out == ceil_div(n * f.up, f.down), "fw_resample: n_out is %lld, %lld samples at %d Hz give %lld at %d Hz",
               (long long)n_out, (long long)n, rate_in, (long long)ceil_div(n * f.up, f.down), rate_out);
  FW_CHECK_ARG(n == 0 || (x && out), "fw_resample: null argument");
  if (n == 0) return FW_OK;
  if (f.up == 1 && f.down == 1) {   // same rate: a copy (audio.py::resample returns its input), i.e. the one-tap filter {1}
    f.half = 0;
    f.h.assign(1, 1.0);
  } else {
    fill(&f, beta);
  }
  return make_plan(f, plan);
}

int check_device(int32_t device_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_index < 0 || device_index >= ndev) {
    fw::set_error("fw_resample_dev: no HIP device %d", device_index);
    return FW_ENODEV;
  }
  return FW_OK;
}

}  // namespace

extern "C" int32_t fw_resample_filter(int32_t rate_in, int32_t rate_out, int32_t taps_per_phase, double beta, double* h,
                                      int64_t* n_h, int32_t* up, int32_t* down) {
  FW_CHECK_ARG(n_h && up && down, "fw_resample_filter: null argument");
  Filter f;
  int rc = design(rate_in, rate_out, taps_per_phase, beta, &f);
  if (rc) return rc;
  *n_h = 2 * f.half + 1;
  *up = f.up;
  *down = f.down;
  if (h) {
    fill(&f, beta);
    for (size_t i = 0; i < f.h.size(); ++i) h[i] = f.h[i];
  }
  return FW_OK;
}

#define RS_TRY(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fw::set_error("%s failed: %s", #call, hipGetErrorString(e_));                          \
      cleanup();                                                                             \
      return e_ == hipErrorOutOfMemory ? FW_ENOMEM : FW_ERUNTIME;                            \
    }                                                                                        \
  } while (0)

extern "C" int32_t fw_resample_dev(int32_t device_index, const float* x, int64_t n, int32_t rate_in, int32_t rate_out,
                                   int32_t taps_per_phase, double beta, int32_t quantize_s16, float* out, int64_t n_out) {
  Plan p;
  int rc = plan_call(x, n, rate_in, rate_out, taps_per_phase, beta, out, n_out, &p);
  if (rc || n == 0) return rc;
  if ((rc = check_device(device_index))) return rc;
  int64_t block = kDefaultBlock;
  if (const char* e = getenv("FWAMD_RESAMPLE_BLOCK")) {
    block = atoll(e);
    FW_CHECK_ARG(block >= 1, "FWAMD_RESAMPLE_BLOCK must be a positive number of outputs (got '%s')", e);
  }
  if (block > kMaxBlock) block = kMaxBlock;
  if (block > n_out) block = n_out;
  const int64_t n_blocks = ceil_div(n_out, block);
  const int64_t in_cap = ceil_div((block - 1) * p.down, p.up) + p.taps + 1;   // floats one block can meet
  FW_HIP(hipSetDevice(device_index));
  double* dtab = nullptr;
  float *din[2] = {nullptr, nullptr}, *dout[2] = {nullptr, nullptr};
  hipStream_t st[2] = {nullptr, nullptr};
  auto cleanup = [&]() {
    for (hipStream_t s : st)
      if (s) (void)hipStreamSynchronize(s);      // (nothing may still read or write the buffers freed below)
    for (void* q : {(void*)dtab, (void*)din[0], (void*)din[1], (void*)dout[0], (void*)dout[1]})
      if (q) (void)hipFree(q);
    for (hipStream_t s : st)
      if (s) (void)hipStreamDestroy(s);
  };
  const int n_sets = n_blocks > 1 ? 2 : 1;
  RS_TRY(hipMalloc(reinterpret_cast<void**>(&dtab), p.table.size() * sizeof(double)));
  for (int s = 0; s < n_sets; ++s) {
    RS_TRY(hipMalloc(reinterpret_cast<void**>(&din[s]), (size_t)in_cap * sizeof(float)));
    RS_TRY(hipMalloc(reinterpret_cast<void**>(&dout[s]), (size_t)block * sizeof(float)));
    RS_TRY(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
  }
  RS_TRY(hipMemcpy(dtab, p.table.data(), p.table.size() * sizeof(double), hipMemcpyHostToDevice));
  // block i lives on stream / buffer pair i & 1: the stream orders its upload after the download of block i - 2
  auto start_block = [&](int64_t i) -> hipError_t {
    const int s = (int)(i & 1);
    const int64_t m_lo = i * block, n_m = n_out - m_lo < block ? n_out - m_lo : block;
    int64_t lo, hi;
    input_span(p, n, m_lo, n_m, &lo, &hi);
    if (hi > lo) {
      hipError_t e = hipMemcpyAsync(din[s], x + lo, (size_t)(hi - lo) * sizeof(float), hipMemcpyHostToDevice, st[s]);
      if (e != hipSuccess) return e;
    }
    launch(p, dtab, din[s], lo, hi - lo, m_lo, n_m, quantize_s16, dout[s], st[s]);
    return hipGetLastError();
  };
  RS_TRY(start_block(0));
  for (int64_t i = 0; i < n_blocks; ++i) {
    if (i + 1 < n_blocks) RS_TRY(start_block(i + 1));
    const int64_t m_lo = i * block, n_m = n_out - m_lo < block ? n_out - m_lo : block;
    RS_TRY(hipMemcpyAsync(out + m_lo, dout[i & 1], (size_t)n_m * sizeof(float), hipMemcpyDeviceToHost, st[i & 1]));
  }
  for (int s = 0; s < n_sets; ++s) RS_TRY(hipStreamSynchronize(st[s]));
  cleanup();
  return FW_OK;
}

// measurement hook (profiles/resample_bench.py): the whole recording resident, every output in ONE launch, timed with
// HIP events over `iters` launches after one warm-up
extern "C" int32_t fw_bench_resample(int32_t device_index, const float* x, int64_t n, int32_t rate_in, int32_t rate_out,
                                     int32_t taps_per_phase, double beta, int32_t quantize_s16, int32_t iters,
                                     float* ms_out) {
  FW_CHECK_ARG(ms_out && iters >= 1 && n > 0, "fw_bench_resample: bad argument");
  Plan p;
  Filter f;
  int rc = design(rate_in, rate_out, taps_per_phase, beta, &f);
  if (rc) return rc;
  const int64_t big = f.up > f.down ? f.up : f.down;
  FW_CHECK_ARG(n <= (INT64_MAX >> 2) / big, "fw_bench_resample: sample count out of range");
  const int64_t n_out = ceil_div(n * f.up, f.down);
  FW_CHECK_ARG(n_out <= kMaxBlock, "fw_bench_resample: at most %lld outputs in one launch", (long long)kMaxBlock);
  if ((rc = plan_call(x, n, rate_in, rate_out, taps_per_phase, beta, x, n_out, &p))) return rc;
  if ((rc = check_device(device_index))) return rc;
  FW_HIP(hipSetDevice(device_index));
  double* dtab = nullptr;
  float *din = nullptr, *dout = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  auto cleanup = [&]() {
    if (st) (void)hipStreamSynchronize(st);
    for (void* q : {(void*)dtab, (void*)din, (void*)dout})
      if (q) (void)hipFree(q);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  };
  RS_TRY(hipMalloc(reinterpret_cast<void**>(&dtab), p.table.size() * sizeof(double)));
  RS_TRY(hipMalloc(reinterpret_cast<void**>(&din), (size_t)n * sizeof(float)));
  RS_TRY(hipMalloc(reinterpret_cast<void**>(&dout), (size_t)n_out * sizeof(float)));
  RS_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  RS_TRY(hipEventCreate(&ev[0]));
  RS_TRY(hipEventCreate(&ev[1]));
  RS_TRY(hipMemcpy(dtab, p.table.data(), p.table.size() * sizeof(double), hipMemcpyHostToDevice));
  RS_TRY(hipMemcpy(din, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  launch(p, dtab, din, 0, n, 0, n_out, quantize_s16, dout, st);
  RS_TRY(hipGetLastError());
  RS_TRY(hipEventRecord(ev[0], st));
  for (int i = 0; i < iters; ++i) launch(p, dtab, din, 0, n, 0, n_out, quantize_s16, dout, st);
  RS_TRY(hipGetLastError());
  RS_TRY(hipEventRecord(ev[1], st));
  RS_TRY(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  RS_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  *ms_out = ms / (float)iters;
  cleanup();
  return FW_OK;
}
#undef RS_TRY
