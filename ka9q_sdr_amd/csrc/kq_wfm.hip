// kq_wfm.hip -- wideband FM stereo decoder bank: broadcast composite -> left / right audio on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_wfm_*): pilot p = h_p * x, u = p / |p|, d[n] = 2 x[n - D] Re(u^2), a = (h_m * x)[n - D],
// s = h_m * d, L / R = g (a +- sigma s) at every Da-th sample, sigma from a per-frame pilot measurement with hysteresis.
// Frames are L samples on a grid shared by every slot, so every count of a call is a closed form of the stream index and
// the host sizes the launches without reading anything back.  State on the device, per slot: a ring of the composite
// (x[n] at n mod Rx) and a ring of the difference signal (d[n] at n mod Rd), long enough that a call's frames find their
// M - 1 + D samples of history and nothing of this call overwrites what it still reads; the frame status and flags of
// the call; the carried stereo state.
//
// k_wfm_ingest  the call's composite samples of each slot's source row into the slot's ring
// k_wfm_pilot   one workgroup per (slot, frame): x's N-window, kq::fft_any<-1> in LDS, times H_p, inverse transform; the L
//               valid samples give d (into the d ring) and, in double, the lag-1 product, C and T of the frame's status
// k_wfm_flags   one lane per slot: the call's frames in order through the hysteresis, status out
// k_wfm_audio   one workgroup per (slot, frame): x delayed by D + j d as one complex window, forward transform, times H_m
//               folded to N / Da bins (exact decimation: the aliases are added), N / Da-point inverse transform, L / R
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_ldsfft.hpp"
#include "kq_slots.hpp"
#include "kq_window.hpp"

namespace {

using kq::FftDim;

constexpr unsigned kMaxSlots = 4096;
constexpr int kMaxN = 16384;
constexpr int kTwLog2 = 14;      // half-circle twiddles of period 16384 serve every power of two <= kMaxN
constexpr int kPer = 16;         // transform points per thread at most (kq::fft_threads)
constexpr double kPilotHz = 19000.0, kAudioHz = 15000.0;

struct WfmPar {  // per slot, written by the host at kq_wfm_set
  int active;
  int force_mono;
  unsigned source;
  float gain;                     // Fc / (2 pi 0.9 deviation_hz)
  float on_db, off_db, min_hz, tol_hz;
  const float2 *hm;               // [N] H_m / N
};

struct WfmGeom {
  int N, L, M, D, Da, Ndec, Lo, skip;  // Lo = L / Da outputs per frame, skip = (M - 1) / Da
  int nthr;
  int Fmax;
  size_t Rx, Rd;
  float Fc;
  FftDim dN, dNdec;
  const float2 *tw;
  const float2 *hp;               // [N] H_p / N
};

struct CallArgs {
  WfmGeom g;
  const WfmPar *par;
  const int *list;                // active slots, ascending
  float *x;                       // [S][Rx]
  float *d;                       // [S][Rd]
  float4 *fst;                    // [S][Fmax] (pilot_hz, pilot_dev_hz, pilot_snr_db, -)
  float *sig;                     // [S][Fmax]
  int *flag;                      // [S]
  uint64_t n0, F0;                // the call's first sample, first frame
  int F;
  // input
  const float *comp;
  size_t src_stride, row_stride;
  unsigned block_len;
  const int *rowmap;              // per list entry: the row of `comp` (host input, staged) or null (par.source)
  size_t xbase;                   // n0 mod Rx
  // output
  float *out;
  size_t ostride;
  kq_wfm_status *st;
  size_t sstride;
};

__device__ __forceinline__ size_t ring_pos(int64_t n, size_t R) {
  int64_t const r = n % (int64_t)R;
  return (size_t)(r < 0 ? r + (int64_t)R : r);
}

__global__ __launch_bounds__(256) void k_wfm_ingest(CallArgs a, size_t ncall) {
  int const li = blockIdx.y, slot = a.list[li];
  size_t const row = a.rowmap ? (size_t)a.rowmap[li] : (size_t)a.par[slot].source;
  const float *src = a.comp + row * a.src_stride;
  float *x = a.x + (size_t)slot * a.g.Rx;
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncall; i += stride) {
    size_t const k = i / a.block_len, j = i - k * a.block_len;
    size_t pos = a.xbase + i;
    if (pos >= a.g.Rx) pos -= a.g.Rx;
    x[pos] = src[k * a.row_stride + j];
  }
}

// sums of three doubles over the workgroup, in a fixed order (every thread gets them)
__device__ void block_sum3(double &u, double &v, double &w, double *red) {
  for (int m = 32; m >= 1; m >>= 1) {
    u += __shfl_xor(u, m);
    v += __shfl_xor(v, m);
    w += __shfl_xor(w, m);
  }
  int const wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[3 * wv] = u;
    red[3 * wv + 1] = v;
    red[3 * wv + 2] = w;
  }
  __syncthreads();
  u = v = w = 0.0;
  for (int k = 0; k < nw; k++) {
    u += red[3 * k];
    v += red[3 * k + 1];
    w += red[3 * k + 2];
  }
}

// buf (natural order, n points) times H, into `d`'s input order for the next transform
__device__ __forceinline__ void mul_reorder(float2 *buf, const float2 *__restrict__ H, int n, const FftDim &d) {
  int const tid = threadIdx.x, nthr = blockDim.x;
  float2 v[kPer];
#pragma unroll
  for (int t = 0; t < kPer; t++) {
    int const k = tid + t * nthr;
    if (k < n) v[t] = kq::cmul(buf[k], H[k]);
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kPer; t++) {
    int const k = tid + t * nthr;
    if (k < n) buf[kq::fft_pos((unsigned)k, d)] = v[t];
  }
}

// dynamic LDS: N float2
__global__ __launch_bounds__(1024) void k_wfm_pilot(CallArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  __shared__ double red[3 * 16];
  WfmGeom const &g = a.g;
  int const slot = a.list[blockIdx.y], fi = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  int64_t const f = (int64_t)(a.F0 + (uint64_t)fi);
  const float *x = a.x + (size_t)slot * g.Rx;
  float *dr = a.d + (size_t)slot * g.Rd;
  // window: x[f L - (M - 1) + i], i < N
  size_t const px = ring_pos(f * g.L - (g.M - 1), g.Rx);
  for (int i = tid; i < g.N; i += nthr) {
    size_t pos = px + i;
    if (pos >= g.Rx) pos -= g.Rx;
    buf[kq::fft_pos((unsigned)i, g.dN)] = make_float2(x[pos], 0.f);
  }
  kq::fft_any<-1>(buf, g.dN, g.tw, kTwLog2);
  mul_reorder(buf, g.hp, g.N, g.dN);
  kq::fft_any<+1>(buf, g.dN, g.tw, kTwLog2);
  // p[f L + i] = buf[M - 1 + i]
  size_t const pd = ring_pos(f * g.L, g.Rd);
  double lx = 0.0, ly = 0.0, tt = 0.0;
  for (int i = tid; i < g.L; i += nthr) {
    int const w = g.M - 1 + i;
    float2 const p = buf[w];
    float const m2 = p.x * p.x + p.y * p.y;
    float const re2 = m2 > 0.f ? (p.x * p.x - p.y * p.y) / m2 : 0.f;  // Re(u^2)
    size_t pos = px + (size_t)(w - g.D);
    if (pos >= g.Rx) pos -= g.Rx;
    size_t q = pd + i;
    if (q >= g.Rd) q -= g.Rd;
    dr[q] = 2.f * x[pos] * re2;
    tt += (double)m2;
    if (i > 0) {
      float2 const o = buf[w - 1];
      lx += (double)p.x * o.x + (double)p.y * o.y;  // p conj(o)
      ly += (double)p.y * o.x - (double)p.x * o.y;
    }
  }
  block_sum3(lx, ly, tt, red);
  double const wh = atan2(ly, lx);  // rad / sample
  double const turns = wh * (0.5 / M_PI);
  double cx = 0.0, cy = 0.0, unused = 0.0;
  for (int i = tid; i < g.L; i += nthr) {
    float2 const p = buf[g.M - 1 + i];
    double t = turns * i;
    t -= rint(t);
    float s, c;
    sincospif(2.f * (float)t, &s, &c);
    cx += (double)p.x * c + (double)p.y * s;  // p exp(-j w i)
    cy += (double)p.y * c - (double)p.x * s;
  }
  block_sum3(cx, cy, unused, red);
  if (tid == 0) {
    double const inv = 1.0 / g.L;
    double const C = (cx * cx + cy * cy) * inv * inv, T = tt * inv;
    double const k = g.Fc * (0.5 / M_PI);
    float4 r;
    r.x = (float)(wh * k);
    r.y = (float)(2.0 * sqrt(C) * k);
    r.z = T - C > 0.0 ? (float)(10.0 * log10(C / (T - C))) : 100.f;
    r.w = 0.f;
    a.fst[(size_t)slot * g.Fmax + fi] = r;
  }
}

// one lane per slot: the call's frames in order
__global__ __launch_bounds__(64) void k_wfm_flags(CallArgs a, int nlist) {
  int const li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nlist) return;
  int const slot = a.list[li];
  WfmPar const &p = a.par[slot];
  int on = a.flag[slot];
  for (int fi = 0; fi < a.F; fi++) {
    float4 const r = a.fst[(size_t)slot * a.g.Fmax + fi];
    bool const rest = r.y >= p.min_hz && fabsf(r.x - (float)kPilotHz) <= p.tol_hz;
    on = on ? (rest && !(r.z < p.off_db)) : (rest && r.z >= p.on_db);
    int const sg = p.force_mono ? 0 : on;
    a.sig[(size_t)slot * a.g.Fmax + fi] = (float)sg;
    if (a.st) {
      kq_wfm_status s;
      s.pilot_hz = r.x;
      s.pilot_dev_hz = r.y;
      s.pilot_snr_db = r.z;
      s.stereo = sg;
      a.st[(size_t)slot * a.sstride + fi] = s;
    }
  }
  a.flag[slot] = on;
}

// dynamic LDS: N float2
__global__ __launch_bounds__(1024) void k_wfm_audio(CallArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  WfmGeom const &g = a.g;
  int const slot = a.list[blockIdx.y], fi = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  WfmPar const &p = a.par[slot];
  int64_t const f = (int64_t)(a.F0 + (uint64_t)fi);
  const float *x = a.x + (size_t)slot * g.Rx;
  const float *dr = a.d + (size_t)slot * g.Rd;
  // z[i] = x[f L - (M - 1) + i - D] + j d[f L - (M - 1) + i]
  size_t const px = ring_pos(f * g.L - (g.M - 1) - g.D, g.Rx), pd = ring_pos(f * g.L - (g.M - 1), g.Rd);
  for (int i = tid; i < g.N; i += nthr) {
    size_t u = px + i, v = pd + i;
    if (u >= g.Rx) u -= g.Rx;
    if (v >= g.Rd) v -= g.Rd;
    buf[kq::fft_pos((unsigned)i, g.dN)] = make_float2(x[u], dr[v]);
  }
  kq::fft_any<-1>(buf, g.dN, g.tw, kTwLog2);
  // Y[k] = sum_r Z[k + r Ndec] H_m[k + r Ndec], k < Ndec: the N-point output at every Da-th sample
  {
    float2 v[kPer];
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const k = tid + t * nthr;
      if (k < g.Ndec) {
        float2 acc = make_float2(0.f, 0.f);
        for (int r = 0; r < g.Da; r++) {
          int const kk = k + r * g.Ndec;
          acc = kq::cadd(acc, kq::cmul(buf[kk], p.hm[kk]));
        }
        v[t] = acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const k = tid + t * nthr;
      if (k < g.Ndec) buf[kq::fft_pos((unsigned)k, g.dNdec)] = v[t];
    }
  }
  kq::fft_any<+1>(buf, g.dNdec, g.tw, kTwLog2);
  if (!a.out) return;
  float const sg = a.sig[(size_t)slot * g.Fmax + fi], gain = p.gain;
  float *o = a.out + (size_t)slot * a.ostride + (size_t)fi * g.Lo * 2;
  for (int m = tid; m < g.Lo; m += nthr) {
    float2 const y = buf[g.skip + m];  // (a, s)
    o[2 * m] = gain * (y.x + sg * y.y);
    o[2 * m + 1] = gain * (y.x - sg * y.y);
  }
}

// ---- host design, in double ----------------------------------------------------------------------------------------
using kq::bin_hz;
using kq::cd;
using kq::window_design;

std::vector<float2> design_mono(int N, int M, double beta, double Fc, double tau_us) {
  std::vector<cd> R((size_t)N, 0.0);
  double const tau = tau_us * 1e-6;
  for (int k = 0; k < N; k++) {
    double const f = bin_hz(k, N, Fc);
    if (std::fabs(f) <= kAudioHz) R[k] = 1.0 / cd(1.0, 2.0 * M_PI * f * tau);
  }
  return window_design(R, M, beta);
}
std::vector<float2> design_pilot(int N, int M, double beta, double Fc, double bw) {
  std::vector<cd> R((size_t)N, 0.0);
  for (int k = 0; k < N; k++)
    if (std::fabs(bin_hz(k, N, Fc) - kPilotHz) <= bw / 2) R[k] = 1.0;
  return window_design(R, M, beta);
}

}  // namespace

struct kq_wfm_bank : kq::HostSide {
  kq_wfm_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  WfmGeom g{};
  uint64_t n_cur = 0;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<WfmPar> slots;
    std::map<float, float2 *> hm;        // one H_m per de-emphasis
    float *x = nullptr, *diff = nullptr, *sig = nullptr;
    float4 *fst = nullptr;
    int *flag = nullptr;
    float2 *hp = nullptr;
    // host-memory calls
    float *out = nullptr;
    kq_wfm_status *st = nullptr;
  } d;
};

namespace {

int make_device(kq_wfm_bank *b) {
  kq_wfm_config const &c = b->cfg;
  WfmGeom &g = b->g;
  auto &d = b->d;
  bool okN = false, okD = false;
  g.dN = kq::fft_dim(g.N, &okN);
  g.dNdec = kq::fft_dim(g.Ndec, &okD);
  if (!okN || !okD) {
    kq_internal_set_error("kq_wfm: no transform plan for N %d / N / Da %d", g.N, g.Ndec);
    return -1;
  }
  if (b->open_stream(c.stream)) return -1;
  size_t const S = c.max_slots;
  if (!(g.tw = kq::half_twiddles(kTwLog2))) {  // shared, not the bank's to free
    kq_internal_set_error("kq_wfm: no twiddle table of period 2^%d", kTwLog2);
    return -1;
  }
  std::vector<float2> hp = design_pilot(g.N, g.M, c.kaiser_beta, c.comp_rate, c.pilot_bw);
  if (b->alloc(&d.hp, hp.size()) || d.slots.alloc(*b, S) || b->alloc(&d.x, S * g.Rx) || b->alloc(&d.diff, S * g.Rd) ||
      b->alloc(&d.fst, S * g.Fmax) || b->alloc(&d.sig, S * g.Fmax) || b->alloc(&d.flag, S, true))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.hp, hp.data(), hp.size() * sizeof(float2), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  g.hp = d.hp;
  return 0;
}

// zero history, flag off (the stream is idle: callers synchronised it)
int cold_start(kq_wfm_bank *b, unsigned s) {
  KQ_TRY(hipMemsetAsync(b->d.x + (size_t)s * b->g.Rx, 0, b->g.Rx * sizeof(float), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.diff + (size_t)s * b->g.Rd, 0, b->g.Rd * sizeof(float), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.flag + s, 0, sizeof(int), b->stream));
  return 0;
}

const char *check_params(const kq_wfm_params *p) {
  if (!std::isfinite(p->deviation_hz) || p->deviation_hz <= 0) return "deviation_hz must be finite and positive";
  if (!std::isfinite(p->deemph_us) || p->deemph_us < 0 || p->deemph_us > 1e4) return "deemph_us must be 0..10000";
  if (!std::isfinite(p->pilot_on_db) || !std::isfinite(p->pilot_off_db)) return "pilot_on_db / pilot_off_db must be finite";
  if (p->pilot_off_db > p->pilot_on_db) return "pilot_off_db must not exceed pilot_on_db";
  if (!std::isfinite(p->pilot_min_hz) || p->pilot_min_hz < 0) return "pilot_min_hz must be finite and >= 0";
  if (!std::isfinite(p->pilot_tol_hz) || p->pilot_tol_hz < 0) return "pilot_tol_hz must be finite and >= 0";
  return nullptr;
}

}  // namespace

extern "C" {

kq_wfm_bank *kq_wfm_create(const kq_wfm_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_wfm_create: null config");
    return nullptr;
  }
  double const Fc = cfg->comp_rate;
  unsigned const Da = cfg->decimate, L = cfg->L, M = cfg->M;
  if (cfg->comp_rate < 128000) {
    kq_internal_set_error("kq_wfm_create: comp_rate %d must be >= 128000", cfg->comp_rate);
    return nullptr;
  }
  if (Da == 0 || Fc / Da < 32000) {
    kq_internal_set_error("kq_wfm_create: decimate %u gives an output rate below 32000 (comp_rate %d)", Da, cfg->comp_rate);
    return nullptr;
  }
  if (M < 3 || !(M & 1)) {
    kq_internal_set_error("kq_wfm_create: M %u must be odd and >= 3", M);
    return nullptr;
  }
  if (L == 0 || L % Da || (M - 1) % Da) {
    kq_internal_set_error("kq_wfm_create: decimate %u must divide L %u and M - 1 %u", Da, L, M - 1);
    return nullptr;
  }
  unsigned long const N = (unsigned long)L + M - 1;
  if (N > (unsigned long)kMaxN || (N & 1) || !kq::fft_size_ok((int)N)) {
    kq_internal_set_error("kq_wfm_create: N = L + M - 1 = %lu must be even, 2^a 3^b 5^c 7^d and <= %d", N, kMaxN);
    return nullptr;
  }
  if (!std::isfinite(cfg->kaiser_beta) || cfg->kaiser_beta < 0) {
    kq_internal_set_error("kq_wfm_create: kaiser_beta must be finite and >= 0");
    return nullptr;
  }
  if (!std::isfinite(cfg->pilot_bw) || cfg->pilot_bw <= 0) {
    kq_internal_set_error("kq_wfm_create: pilot_bw must be finite and positive");
    return nullptr;
  }
  double const trans = 2.0 * Fc * std::sqrt(1.0 + (double)cfg->kaiser_beta * cfg->kaiser_beta) / M;
  if (kAudioHz + trans > kPilotHz - cfg->pilot_bw / 2.0) {
    kq_internal_set_error("kq_wfm_create: 15 kHz + transition band %.0f Hz does not fit below 19 kHz - pilot_bw / 2 (longer M, "
                          "lower kaiser_beta or a narrower pilot_bw)", trans);
    return nullptr;
  }
  if (cfg->max_slots == 0 || cfg->max_slots > kMaxSlots) {
    kq_internal_set_error("kq_wfm_create: max_slots %u must be 1..%u", cfg->max_slots, kMaxSlots);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_wfm_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  kq_wfm_bank *b = new kq_wfm_bank;
  b->cfg = *cfg;
  WfmGeom &g = b->g;
  g.N = (int)N;
  g.L = (int)L;
  g.M = (int)M;
  g.D = (int)(M - 1) / 2;
  g.Da = (int)Da;
  g.Ndec = (int)(N / Da);
  g.Lo = (int)(L / Da);
  g.skip = (int)((M - 1) / Da);
  g.nthr = kq::fft_threads(g.N);
  g.Fmax = (int)((cfg->max_samples + L - 1) / L);
  g.Rx = cfg->max_samples + L - 1 + (M - 1) + g.D;
  g.Rd = (size_t)g.Fmax * L + M - 1;
  g.Fc = (float)Fc;
  return b;
}

int kq_wfm_destroy(kq_wfm_bank *b) { return kq::destroy_bank(b, "kq_wfm_destroy"); }

int kq_wfm_set(kq_wfm_bank *b, unsigned slot, const kq_wfm_params *p) {
  if (!kq::set_args_ok("kq_wfm_set", slot, p, kMaxSlots)) return -1;
  if (const char *why = check_params(p)) {
    kq_internal_set_error("kq_wfm_set: %s", why);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_wfm_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("kq_wfm_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  auto it = b->d.hm.find(p->deemph_us);
  if (it == b->d.hm.end()) {
    std::vector<float2> h = design_mono(b->g.N, b->g.M, b->cfg.kaiser_beta, b->cfg.comp_rate, p->deemph_us);
    float2 *d = nullptr;
    if (b->alloc(&d, h.size())) return -1;
    KQ_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice));
    it = b->d.hm.emplace(p->deemph_us, d).first;
  }
  WfmPar np{};
  np.active = 1;
  np.force_mono = p->force_mono ? 1 : 0;
  np.source = p->source;
  np.gain = (float)((double)b->cfg.comp_rate / (2.0 * M_PI * 0.9 * (double)p->deviation_hz));
  np.on_db = p->pilot_on_db;
  np.off_db = p->pilot_off_db;
  np.min_hz = p->pilot_min_hz;
  np.tol_hz = p->pilot_tol_hz;
  np.hm = it->second;
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_wfm_remove(kq_wfm_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_wfm_remove"); }

int kq_wfm_process(kq_wfm_bank *b, const float *comp, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, float *out, size_t out_stride, kq_wfm_status *status,
                   size_t status_stride) {
  if (!b) {
    kq_internal_set_error("kq_wfm_process: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_wfm_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  WfmGeom &g = b->g;
  uint64_t const n0 = b->n_cur, n1 = n0 + ncall, F0 = n0 / (uint64_t)g.L;
  int const F = (int)(n1 / (uint64_t)g.L - F0);
  if (out && out_stride < (size_t)2 * F * g.Lo) {
    kq_internal_set_error("kq_wfm_process: out_stride %zu < 2 F L / decimate = %zu", out_stride, (size_t)2 * F * g.Lo);
    return -1;
  }
  if (status && status_stride < (size_t)F) {
    kq_internal_set_error("kq_wfm_process: status_stride %zu < F = %d", status_stride, F);
    return -1;
  }
  kq::CallWork const work = kq::call_work(b, "kq_wfm_process", ncall, comp, "comp");
  if (work == kq::CALL_IDLE) {
    b->n_cur = n1;
    return F;
  }
  if (work != kq::CALL_RUN) return work;
  kq::DeviceScope dev_scope_(b->cfg.device);
  auto &d = b->d;
  size_t const S = b->cfg.max_slots, nlist = d.slots.all.size();
  CallArgs a{};
  a.g = g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.x = d.x;
  a.d = d.diff;
  a.fst = d.fst;
  a.sig = d.sig;
  a.flag = d.flag;
  a.n0 = n0;
  a.F0 = F0;
  a.F = F;
  a.block_len = block_len;
  a.xbase = (size_t)(n0 % (uint64_t)g.Rx);
  if (on_device) {
    a.comp = comp;
    a.src_stride = src_stride;
    a.row_stride = row_stride;
    a.rowmap = nullptr;
    a.out = out;
    a.ostride = out_stride;
    a.st = status;
    a.sstride = status_stride;
  } else {
    kq::Staged in;
    if (d.slots.stage_rows(*b, comp, sizeof(float), src_stride, row_stride, block_len, nblocks,
                           b->cfg.max_samples * sizeof(float), &in))
      return -1;
    a.comp = static_cast<const float *>(in.src);
    a.src_stride = in.src_stride;
    a.row_stride = in.row_stride;
    a.rowmap = in.rowmap;
    if (out && !d.out && b->alloc(&d.out, S * 2 * (size_t)g.Fmax * g.Lo)) return -1;
    if (status && !d.st && b->alloc(&d.st, S * (size_t)g.Fmax)) return -1;
    a.out = out ? d.out : nullptr;
    a.ostride = 2 * (size_t)g.Fmax * g.Lo;
    a.st = status ? d.st : nullptr;
    a.sstride = g.Fmax;
  }
  {
    unsigned const chunks = (unsigned)std::min<size_t>((ncall + 255) / 256, 1024);
    hipLaunchKernelGGL(k_wfm_ingest, dim3(chunks, (unsigned)nlist), dim3(256), 0, b->stream, a, ncall);
    KQ_TRY(hipGetLastError());
  }
  if (F > 0) {
    size_t const lds = (size_t)g.N * sizeof(float2);
    kq::ensure_dynamic_lds((const void *)k_wfm_pilot, lds);
    kq::ensure_dynamic_lds((const void *)k_wfm_audio, lds);
    hipLaunchKernelGGL(k_wfm_pilot, dim3((unsigned)F, (unsigned)nlist), dim3(g.nthr), lds, b->stream, a);
    KQ_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wfm_flags, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, b->stream, a, (int)nlist);
    KQ_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wfm_audio, dim3((unsigned)F, (unsigned)nlist), dim3(g.nthr), lds, b->stream, a);
    KQ_TRY(hipGetLastError());
  }
  if (!on_device) {
    // the rows of the active slots; with no frame completed there is nothing to copy
    auto back = [&](size_t s0, size_t n) {
      if (out && kq::copy_rows_back(*b, out, out_stride, d.out, a.ostride, (size_t)2 * F * g.Lo, sizeof(float), s0, n)) return -1;
      if (status && kq::copy_rows_back(*b, status, status_stride, d.st, a.sstride, (size_t)F, sizeof(kq_wfm_status), s0, n))
        return -1;
      return 0;
    };
    if (F > 0 && d.slots.for_runs(back)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  b->n_cur = n1;  // only once everything is queued: a call that fails leaves the stream index where it was
  return F;
}

int kq_wfm_sync(kq_wfm_bank *b) { return kq::sync_bank(b, "kq_wfm_sync"); }

int kq_wfm_reset(kq_wfm_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_wfm_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  for (int s : b->d.slots.all)
    if (cold_start(b, (unsigned)s)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // extern "C"
