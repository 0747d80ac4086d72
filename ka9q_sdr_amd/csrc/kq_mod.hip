// kq_mod.hip -- modulator bank: many modulate.c stations summed into one wideband I/Q stream on gfx950.
//
// Per station and block of L output samples, what modulate.c:131-163 does with the filter + osc API the other way round:
//   modulate.c:136-145  L / I audio samples zero-stuffed by I into the REAL input of an overlap-save filter
//   modulate.c:113-130  response: gain I / N between the edges, window_filter(L, M, response, beta)
//   filter.c:206-216    REAL in, COMPLEX out, decimate 1: G[k] = H[k] X[k] on every bin (X is conjugate symmetric)
//   modulate.c:149-153  + carrier
//   modulate.c:155-157  * step_osc(&osc) * amplitude  (osc.c:22-59 in closed form: phase in double turns)
// FM (beyond the reference): the real part m[n] of the filter output drives theta[n] = theta[n-1] + 2 pi (deviation / Fs) m[n],
// the baseband is exp(i theta[n]), then the same mix.
//
// The zero-stuffed window of N samples holds Na = N / I audio samples at every I-th place (I divides L and M - 1), so its
// N-point spectrum is the Na-point spectrum of those samples repeated I times: the forward transform per station-block is
// Na points, the inverse a full N points (the Kaiser-windowed response has no zero bins to prune).
//
// k_mod_synth: one workgroup per group of G consecutive slots walks the call's blocks in order; per block it runs its
//   stations one after the other through LDS and adds each one's mixed output into the group's partial sum of the block,
//   in place (each thread reads and writes only its own samples; no float atomics).  Oscillator and FM phase advance once per block (not per call), so the bits do not depend
//   on how the blocks are split into calls.
// k_mod_reduce: per output sample, the partials of groups 0, 1, 2, ... in that order; fused cf32 / int16 conversion.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_ldsfft.hpp"

namespace {

using kq::FftDim;

constexpr int kMaxN = 16384;
constexpr unsigned kMaxStations = 65536;
constexpr unsigned kGroups = 256;        // workgroups a full bank is split into (one per CU of an MI355X); G = ceil(S / 256)
constexpr float kS16Scale = (float)(1. / SHRT_MAX);  // modulate.c:24

struct ModParam {   // per slot, written by the host
  int active;
  int type;         // enum kq_mod_type
  int resp;         // index into the response table
  int moving;       // set_osc's freq != 0 (osc.c:44: a zero frequency neither advances nor sweeps)
  float carrier;    // modulate.c:149-153 (linear only)
  float amp;        // 10^(dBFS/20), modulate.c:105
  double dev;       // FM deviation / Fs: theta advance in turns per unit of m[n]
};
struct ModOsc {     // per slot, advanced by the device once per block
  double p;         // phase in turns at the next block's first sample (the phasor of osc.c)
  double f, r;      // cycles / sample, cycles / sample^2 (osc.c:28-33)
  double theta;     // FM phase in turns at the end of the last block
};

struct SynthArgs {
  const ModParam *par;
  ModOsc *osc;
  const float2 *resp;   // [R][N]
  float *hist;          // [S][Hn] audio samples of the last window not yet consumed
  const void *pcm;      // row s at pcm + s * stride elements
  int fmt;              // KQ_PCM_F32 / KQ_PCM_S16
  size_t stride;
  float2 *part;         // [groups][nblocks][L]
  float2 *aspec;        // [groups][Na] scratch: one station's audio spectrum
  int S, G, nblocks;
  int L, M, N, Na, Hn, La;
  FftDim dN, dA;
  const float2 *tw;     // half circle, period 1 << tw_log2 >= N (powers of two only)
  int tw_log2;
};

__device__ __forceinline__ float pcm_sample(const SynthArgs &a, int s, int idx) {
  size_t const off = (size_t)s * a.stride + (size_t)idx;
  if (a.fmt == KQ_PCM_S16) return (float)reinterpret_cast<const int16_t *>(a.pcm)[off] * kS16Scale;  // modulate.c:141
  return reinterpret_cast<const float *>(a.pcm)[off];
}

// dynamic LDS: N float2, then the group's G ModParam and G ModOsc (synth_lds_bytes)
__global__ __launch_bounds__(1024) void k_mod_synth(SynthArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  ModParam *spar = reinterpret_cast<ModParam *>(buf + a.N);
  ModOsc *sosc = reinterpret_cast<ModOsc *>(spar + a.G);
  __shared__ double wsum[16];
  int const g = blockIdx.x, T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int const s0 = g * a.G, ns = min(a.G, a.S - s0);
  for (int j = tid; j < ns; j += T) {
    spar[j] = a.par[s0 + j];
    sosc[j] = a.osc[s0 + j];
  }
  __syncthreads();

  for (int b = 0; b < a.nblocks; b++) {
    // the group's sum of block b, added up in place: every thread reads and writes only its own samples
    float2 *dst = a.part + ((size_t)g * a.nblocks + b) * a.L;
    bool first = true;
    for (int j = 0; j < ns; j++) {
      ModParam const p = spar[j];
      if (!p.active) continue;
      int const s = s0 + j;
      ModOsc const o = sosc[j];
      // audio window of this block: [hist | pcm] from b * La on, Na samples, digit-reversed for the Na-point transform
      const float *h = a.hist + (size_t)s * a.Hn;
      for (int q = tid; q < a.Na; q += T) {
        int const idx = b * a.La + q;
        float const v = idx < a.Hn ? h[idx] : pcm_sample(a, s, idx - a.Hn);
        buf[kq::fft_pos((unsigned)q, a.dA)] = make_float2(v, 0.f);
      }
      kq::fft_any<-1>(buf, a.dA, a.tw, a.tw_log2);
      // the Na-point spectrum A to the group's scratch row (the N-point input below lands on top of it in LDS), then
      // G[k] = H[k] A[k mod Na] into the N-point inverse transform's digit-reversed order
      float2 *A = a.aspec + (size_t)g * a.Na;
      for (int q = tid; q < a.Na; q += T) A[q] = buf[q];
      __threadfence_block();
      __syncthreads();
      const float2 *H = a.resp + (size_t)p.resp * a.N;
      for (int k = tid; k < a.N; k += T) buf[kq::fft_pos((unsigned)k, a.dN)] = kq::cmul(H[k], A[k % a.Na]);
      kq::fft_any<+1>(buf, a.dN, a.tw, a.tw_log2);  // output.c = buf[M - 1 ...] (filter.c:250, create_filter_output)
      bool const fm = p.type == KQ_MOD_FM;
      if (fm) {
        // theta over the block: each thread a contiguous run of samples, runs joined by a scan in double
        int const P = (a.L + T - 1) / T, n0 = min(a.L, tid * P), n1 = min(a.L, n0 + P);
        double loc = 0;
        for (int n = n0; n < n1; n++) loc += (double)buf[a.M - 1 + n].x;
        double inc = loc;
        for (int d = 1; d < 64; d <<= 1) {
          double const t = __shfl_up(inc, d);
          if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        double run = inc - loc;
        for (int w = 0; w < wave; w++) run += wsum[w];
        for (int n = n0; n < n1; n++) {
          run += (double)buf[a.M - 1 + n].x;
          buf[a.M - 1 + n] = kq::phasor_turns(o.theta + p.dev * run);
        }
        if (n1 == a.L && n0 < a.L) {  // the thread holding the block's last sample carries theta, wrapped
          double const th = o.theta + p.dev * run;
          sosc[j].theta = th - rint(th);
        }
        __syncthreads();
      }
      for (int n = tid; n < a.L; n += T) {
        float2 const y = buf[a.M - 1 + n];
        float2 const bb = fm ? y : make_float2(y.x + p.carrier, y.y);
        double const ph = p.moving ? o.p + (double)n * (o.f + 0.5 * o.r * (double)(n - 1)) : o.p;
        float2 const w = kq::phasor_turns(ph);
        float2 const v = kq::cmul(bb, make_float2(w.x * p.amp, w.y * p.amp));
        dst[n] = first ? v : kq::cadd(dst[n], v);
      }
      first = false;
      // the oscillator at the next block's start: every thread holds its copy `o` since before the first barrier of this
      // station-block, and the barrier below orders the write before the next block's read
      if (tid == 0 && p.moving) {
        double const Ld = (double)a.L;
        double const np = o.p + Ld * (o.f + 0.5 * o.r * (Ld - 1.0));
        sosc[j].p = np - rint(np);
        sosc[j].f = o.f + o.r * Ld;
      }
      __syncthreads();  // buf is the next station's
    }
    if (first)  // no station on the air in this group
      for (int n = tid; n < a.L; n += T) dst[n] = make_float2(0.f, 0.f);
  }
  __syncthreads();
  for (int j = tid; j < ns; j += T)
    if (spar[j].active) a.osc[s0 + j] = sosc[j];
  // the next call's history: the last Hn samples of [hist | pcm], staged through LDS (the two may overlap)
  float *stage = reinterpret_cast<float *>(buf);
  int const consumed = a.nblocks * a.La;
  for (int j = 0; j < ns; j++) {
    if (!spar[j].active) continue;
    int const s = s0 + j;
    float *h = a.hist + (size_t)s * a.Hn;
    for (int q = tid; q < a.Hn; q += T) {
      int const idx = consumed + q;
      stage[q] = idx < a.Hn ? h[idx] : pcm_sample(a, s, idx - a.Hn);
    }
    __syncthreads();
    for (int q = tid; q < a.Hn; q += T) h[q] = stage[q];
    __syncthreads();
  }
}

// out = sum over groups 0, 1, ... of part (that order); int16: trunc(x * 32767) as modulate.c:160-163, saturated
__global__ __launch_bounds__(256) void k_mod_reduce(const float2 *__restrict__ part, int groups, size_t total, float2 *__restrict__ out,
                                                    int16_t *__restrict__ s16) {
  size_t const n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= total) return;
  float2 v = part[n];
  for (int g = 1; g < groups; g++) v = kq::cadd(v, part[(size_t)g * total + n]);
  if (out) out[n] = v;
  if (s16) {
    float const x = fminf(fmaxf(v.x * (float)SHRT_MAX, -32768.f), 32767.f);
    float const y = fminf(fmaxf(v.y * (float)SHRT_MAX, -32768.f), 32767.f);
    s16[2 * n] = (int16_t)x;
    s16[2 * n + 1] = (int16_t)y;
  }
}

size_t synth_lds_bytes(int N, int G) { return (size_t)N * sizeof(float2) + (size_t)G * (sizeof(ModParam) + sizeof(ModOsc)); }

struct RespKey {
  float low, high, beta;
  bool operator<(const RespKey &o) const {
    return std::memcmp(this, &o, sizeof *this) < 0;
  }
};

}  // namespace

struct kq_mod_bank : kq::HostSide {
  kq_mod_config cfg;
  int N = 0, Na = 0, Hn = 0, La = 0, G = 1, groups = 0, threads = 64;
  FftDim dN{}, dA{};
  // host mirror
  std::vector<ModParam> par;
  std::vector<kq_station_config> st;
  // responses shared by every station with the same (low, high, beta)
  std::map<RespKey, int> resp_of;
  std::vector<RespKey> resp_key;
  std::vector<int> resp_refs;
  int resp_cap = 0;
  // device
  const float2 *tw = nullptr;  // kq::half_twiddles(tw_log2): shared, not the bank's to free
  int tw_log2 = 0;
  ModParam *d_par = nullptr;
  ModOsc *d_osc = nullptr;
  float *d_hist = nullptr;
  float2 *d_resp = nullptr, *d_part = nullptr, *d_aspec = nullptr, *d_out = nullptr;
  int16_t *d_s16 = nullptr;
  char *d_pcm = nullptr;
  size_t pcm_bytes = 0;
};

namespace {

int mod_alloc(kq_mod_bank *b) {
  kq_mod_config const &c = b->cfg;
  kq::DeviceScope dev_scope_(c.device);
  if (b->open_stream(c.stream)) return -1;
  bool okN = false, okA = false;
  b->dN = kq::fft_dim(b->N, &okN);
  b->dA = kq::fft_dim(b->Na, &okA);
  if (!okN || !okA) {
    kq_internal_set_error("kq_mod_create: no transform plan for N = %d / Na = %d", b->N, b->Na);
    return -1;
  }
  b->tw_log2 = 1;
  while ((1 << b->tw_log2) < b->N) b->tw_log2++;
  if (!(b->tw = kq::half_twiddles(b->tw_log2))) {
    kq_internal_set_error("kq_mod_create: no twiddle table of period 2^%d", b->tw_log2);
    return -1;
  }
  size_t const S = c.max_stations, L = c.L;
  if (b->alloc(&b->d_par, S, true) || b->alloc(&b->d_osc, S, true) || b->alloc(&b->d_hist, std::max<size_t>(1, S * b->Hn)) ||
      b->alloc(&b->d_part, (size_t)b->groups * c.max_blocks * L) || b->alloc(&b->d_aspec, (size_t)b->groups * b->Na) ||
      b->alloc(&b->d_out, (size_t)c.max_blocks * L) || b->alloc(&b->d_s16, (size_t)c.max_blocks * L * 2))
    return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  b->par.assign(S, ModParam{});
  b->st.assign(S, kq_station_config{});
  return 0;
}

// modulate.c:113-130 for any I: gain I / N where low <= f <= high, f in float as the reference evaluates it
int design_station_response(kq_mod_bank *b, const RespKey &k, std::vector<kq::cfloat> &r) {
  int const N = b->N, Fs = b->cfg.samprate;
  r.assign(N, kq::cfloat(0.f, 0.f));
  float const gain = (float)((double)b->cfg.interp / N);
  for (int i = 0; i < N; i++) {
    float f = Fs * ((float)i / N);
    if (f > Fs / 2) f -= Fs;
    if (f >= k.low && f <= k.high) r[i] = gain;
  }
  if (kq::window_filter((int)b->cfg.L, (int)b->cfg.M, r, k.beta) != 0) {
    kq_internal_set_error("kq_mod_set_station: response design failed");
    return -1;
  }
  return 0;
}

// index of the response for `k`, designed and uploaded if no station uses it yet; -1 on failure
int acquire_response(kq_mod_bank *b, const RespKey &k) {
  auto it = b->resp_of.find(k);
  if (it != b->resp_of.end()) {
    b->resp_refs[it->second]++;
    return it->second;
  }
  std::vector<kq::cfloat> r;
  if (design_station_response(b, k, r)) return -1;
  int idx = -1;
  for (size_t i = 0; i < b->resp_refs.size(); i++)
    if (b->resp_refs[i] == 0) {
      idx = (int)i;
      b->resp_of.erase(b->resp_key[i]);
      break;
    }
  if (idx < 0) {
    idx = (int)b->resp_refs.size();
    if (idx >= b->resp_cap) {  // grow the table: queued kernels read the old one, so wait for them first
      int const cap = std::max(4, 2 * b->resp_cap);
      float2 *nr = nullptr;
      KQ_TRY(hipStreamSynchronize(b->stream));
      if (b->alloc(&nr, (size_t)cap * b->N)) return -1;
      if (b->resp_cap)
        KQ_TRY(hipMemcpyAsync(nr, b->d_resp, (size_t)b->resp_cap * b->N * sizeof(float2), hipMemcpyDeviceToDevice, b->stream));
      KQ_TRY(hipStreamSynchronize(b->stream));
      b->release(&b->d_resp);
      b->d_resp = nr;
      b->resp_cap = cap;
    }
    b->resp_refs.push_back(0);
    b->resp_key.push_back(k);
  }
  // stream order: kernels queued before this call still read the slot's old contents
  KQ_TRY(hipMemcpyAsync(b->d_resp + (size_t)idx * b->N, r.data(), (size_t)b->N * sizeof(float2), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  b->resp_refs[idx] = 1;
  b->resp_key[idx] = k;
  b->resp_of[k] = idx;
  return idx;
}

void release_response(kq_mod_bank *b, int idx) {
  if (idx >= 0 && idx < (int)b->resp_refs.size() && b->resp_refs[idx] > 0) b->resp_refs[idx]--;
}

RespKey key_of(const kq_station_config &c) {
  RespKey k;
  std::memset(&k, 0, sizeof k);
  k.low = c.low;
  k.high = c.high;
  k.beta = c.kaiser_beta;
  return k;
}

int upload_param(kq_mod_bank *b, unsigned slot) {
  KQ_TRY(hipMemcpyAsync(b->d_par + slot, &b->par[slot], sizeof(ModParam), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int highest_active(const kq_mod_bank *b) {
  for (int s = (int)b->par.size() - 1; s >= 0; s--)
    if (b->par[s].active) return s;
  return -1;
}

}  // namespace

extern "C" {

kq_mod_bank *kq_mod_create(const kq_mod_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_mod_create: null config");
    return nullptr;
  }
  unsigned const L = cfg->L, M = cfg->M, I = cfg->interp;
  unsigned long const N = (unsigned long)L + M - 1;
  if (cfg->samprate <= 0 || L == 0 || M == 0) {
    kq_internal_set_error("kq_mod_create: samprate, L and M must be positive");
    return nullptr;
  }
  if (N > (unsigned long)kMaxN || (N & 1) || !kq::fft_size_ok((int)N)) {
    kq_internal_set_error("kq_mod_create: N = L + M - 1 = %lu must be even and 2^a 3^b 5^c 7^d up to %d", N, kMaxN);
    return nullptr;
  }
  if (I == 0 || L % I || (M - 1) % I) {
    kq_internal_set_error("kq_mod_create: interp %u must be >= 1 and divide L = %u and M - 1 = %u", I, L, M - 1);
    return nullptr;
  }
  if (cfg->max_stations == 0 || cfg->max_stations > kMaxStations || cfg->max_blocks == 0) {
    kq_internal_set_error("kq_mod_create: max_stations must be 1..%u and max_blocks positive", kMaxStations);
    return nullptr;
  }
  kq_mod_bank *b = new kq_mod_bank;
  b->cfg = *cfg;
  b->N = (int)N;
  b->Na = (int)(N / I);
  b->Hn = (int)((M - 1) / I);
  b->La = (int)(L / I);
  b->G = (int)((cfg->max_stations + kGroups - 1) / kGroups);
  b->groups = (int)((cfg->max_stations + b->G - 1) / b->G);
  b->threads = kq::fft_threads(b->N);
  if (mod_alloc(b) != 0) {
    kq_mod_destroy(b);
    return nullptr;
  }
  return b;
}

int kq_mod_destroy(kq_mod_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mod_destroy: null bank");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  b->close();
  delete b;
  return 0;
}

int kq_mod_set_station(kq_mod_bank *b, unsigned slot, const kq_station_config *c) {
  if (slot >= kMaxStations) {
    kq_internal_set_error("kq_mod_set_station: slot %u is beyond any bank (%u stations at most)", slot, kMaxStations);
    return -1;
  }
  if (!c) {
    kq_internal_set_error("kq_mod_set_station: null station config");
    return -1;
  }
  if (c->mod_type != KQ_MOD_LINEAR && c->mod_type != KQ_MOD_FM) {
    kq_internal_set_error("kq_mod_set_station: unknown mod_type %d", c->mod_type);
    return -1;
  }
  if (!std::isfinite(c->low) || !std::isfinite(c->high) || !std::isfinite(c->carrier) || !std::isfinite(c->kaiser_beta) ||
      !std::isfinite(c->deviation) || !std::isfinite(c->frequency) || !std::isfinite(c->sweep) || !std::isfinite(c->amplitude_dbfs) ||
      c->low > c->high || c->kaiser_beta < 0) {
    kq_internal_set_error("kq_mod_set_station: non-finite parameter, low > high or negative beta");
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_mod_set_station: null bank");
    return -1;
  }
  if (slot >= b->cfg.max_stations) {
    kq_internal_set_error("kq_mod_set_station: slot %u >= max_stations %u", slot, b->cfg.max_stations);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  ModParam &p = b->par[slot];
  bool const was_active = p.active != 0;
  RespKey const k = key_of(*c);
  int idx = p.resp;
  if (!was_active || std::memcmp(&k, &b->resp_key[p.resp], sizeof k) != 0) {  // modulate.c:113-130 on the next block
    int const nidx = acquire_response(b, k);
    if (nidx < 0) return -1;
    if (was_active) release_response(b, p.resp);
    idx = nidx;
  }
  double const Fs = (double)b->cfg.samprate;
  // modulate.c:104-108 then set_osc (osc.c:22-35): a running station keeps its phase, a new one starts at phasor 1
  ModOsc o{};
  o.f = c->frequency / Fs;
  o.r = c->sweep / (Fs * Fs);
  if (!was_active) {
    KQ_TRY(hipMemcpyAsync(b->d_osc + slot, &o, sizeof o, hipMemcpyHostToDevice, b->stream));
    if (b->Hn) KQ_TRY(hipMemsetAsync(b->d_hist + (size_t)slot * b->Hn, 0, (size_t)b->Hn * sizeof(float), b->stream));  // filter.c:76
  } else {
    KQ_TRY(hipMemcpyAsync(&b->d_osc[slot].f, &o.f, 2 * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (c->mod_type == KQ_MOD_FM && p.type != KQ_MOD_FM)  // theta starts at 0 where a station turns to FM
      KQ_TRY(hipMemsetAsync(&b->d_osc[slot].theta, 0, sizeof(double), b->stream));
  }
  p.active = 1;
  p.type = c->mod_type;
  p.resp = idx;
  p.moving = o.f != 0.0;
  p.carrier = c->mod_type == KQ_MOD_FM ? 0.f : c->carrier;
  p.amp = (float)std::pow(10.0, c->amplitude_dbfs / 20.0);
  p.dev = (double)c->deviation / Fs;
  b->st[slot] = *c;
  return upload_param(b, slot);
}

int kq_mod_remove_station(kq_mod_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_mod_remove_station: null bank");
    return -1;
  }
  if (slot >= b->cfg.max_stations || !b->par[slot].active) {
    kq_internal_set_error("kq_mod_remove_station: slot %u holds no station", slot);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  release_response(b, b->par[slot].resp);
  b->par[slot].active = 0;
  return upload_param(b, slot);
}

int kq_mod_process(kq_mod_bank *b, const void *pcm, int pcm_format, size_t stride, unsigned nblocks, int on_device, float *out_cf32,
                   int16_t *out_s16) {
  if (pcm_format != KQ_PCM_F32 && pcm_format != KQ_PCM_S16) {
    kq_internal_set_error("kq_mod_process: unknown pcm_format %d (KQ_PCM_F32 or KQ_PCM_S16)", pcm_format);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_mod_process: null bank");
    return -1;
  }
  if (nblocks == 0 || nblocks > b->cfg.max_blocks) {
    kq_internal_set_error("kq_mod_process: nblocks %u must be 1..max_blocks %u", nblocks, b->cfg.max_blocks);
    return -1;
  }
  if (!out_cf32 && !out_s16) {
    kq_internal_set_error("kq_mod_process: no output");
    return -1;
  }
  int const hi = highest_active(b);
  size_t const nnew = (size_t)nblocks * b->La;
  if (hi >= 0 && (!pcm || stride < nnew)) {
    kq_internal_set_error("kq_mod_process: pcm is null or stride %zu < %zu samples per row", stride, nnew);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  size_t const total = (size_t)nblocks * b->cfg.L;
  float2 *out = on_device ? reinterpret_cast<float2 *>(out_cf32) : (out_cf32 ? b->d_out : nullptr);
  int16_t *s16 = on_device ? out_s16 : (out_s16 ? b->d_s16 : nullptr);
  if (hi < 0) {  // nothing on the air: silence
    if (out) KQ_TRY(hipMemsetAsync(out, 0, total * sizeof(float2), b->stream));
    if (s16) KQ_TRY(hipMemsetAsync(s16, 0, total * 2 * sizeof(int16_t), b->stream));
  } else {
    size_t const esize = pcm_format == KQ_PCM_S16 ? 2 : 4;
    const void *src = pcm;
    size_t row = stride;
    if (!on_device) {  // rows 0 .. hi to the device
      size_t const need = (size_t)(hi + 1) * nnew * esize;
      if (b->grow(&b->d_pcm, &b->pcm_bytes, need)) return -1;
      KQ_TRY(hipMemcpy2DAsync(b->d_pcm, nnew * esize, pcm, stride * esize, nnew * esize, (size_t)hi + 1, hipMemcpyHostToDevice,
                               b->stream));
      src = b->d_pcm;
      row = nnew;
    }
    int const groups = hi / b->G + 1;
    SynthArgs a{};
    a.par = b->d_par;
    a.osc = b->d_osc;
    a.resp = b->d_resp;
    a.hist = b->d_hist;
    a.pcm = src;
    a.fmt = pcm_format;
    a.stride = row;
    a.part = b->d_part;
    a.aspec = b->d_aspec;
    a.S = hi + 1;
    a.G = b->G;
    a.nblocks = (int)nblocks;
    a.L = (int)b->cfg.L;
    a.M = (int)b->cfg.M;
    a.N = b->N;
    a.Na = b->Na;
    a.Hn = b->Hn;
    a.La = b->La;
    a.dN = b->dN;
    a.dA = b->dA;
    a.tw = b->tw;
    a.tw_log2 = b->tw_log2;
    size_t const lds = synth_lds_bytes(b->N, b->G);
    kq::ensure_dynamic_lds((const void *)k_mod_synth, lds);
    hipLaunchKernelGGL(k_mod_synth, dim3(groups), dim3(b->threads), lds, b->stream, a);
    KQ_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mod_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, b->stream, (const float2 *)b->d_part, groups,
                       total, out, s16);
    KQ_TRY(hipGetLastError());
  }
  if (!on_device) {
    if (out_cf32) KQ_TRY(hipMemcpyAsync(out_cf32, b->d_out, total * sizeof(float2), hipMemcpyDeviceToHost, b->stream));
    if (out_s16) KQ_TRY(hipMemcpyAsync(out_s16, b->d_s16, total * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  return 0;
}

int kq_mod_sync(kq_mod_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mod_sync: null bank");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_mod_reset(kq_mod_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mod_reset: null bank");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  size_t const S = b->cfg.max_stations;
  std::vector<ModOsc> o(S);
  for (size_t s = 0; s < S; s++) {
    o[s] = ModOsc{};
    if (b->par[s].active) {
      o[s].f = b->st[s].frequency / (double)b->cfg.samprate;
      o[s].r = b->st[s].sweep / ((double)b->cfg.samprate * b->cfg.samprate);
    }
  }
  KQ_TRY(hipMemcpyAsync(b->d_osc, o.data(), S * sizeof(ModOsc), hipMemcpyHostToDevice, b->stream));
  if (b->Hn) KQ_TRY(hipMemsetAsync(b->d_hist, 0, S * b->Hn * sizeof(float), b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // extern "C"
