// kq_fe.hip -- raw A/D conditioning of the front-end daemons on gfx950: hackrf.c:122-196 (rx_callback) and
// funcube.c:287-390 (the read loop).  int8 / int16 to float, DC removal, I/Q gain balance, I/Q phase correction, and
// the running estimates behind them.  The definition is in ka9q_hip.h (kq_fe_*).
//
// Block k's estimates set block k+1's corrections, but every sum the reference forms over a block is a closed form in five
// integer moments of the raw block and the constants in force at its start.  So a call is three steps:
//   k_fe_moments  the integer moments of every block the call touches: order-independent, hence exact and reproducible
//   k_fe_scan     one lane walks the completed blocks through the recursion in double and writes each block's constants
//   k_fe_apply    the per-sample correction with the constants of the sample's block -- or, for kq_fe_process_decim, the
//                 cascade's first kernel reads the raw samples and applies them itself (kq_decim.hip, RAW instances)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "ka9q_hip.h"
#include "kq_device.hpp"
#include "kq_fe.hpp"
#include "kq_host.hpp"

// the recursion is defined operation by operation (a numpy float64 evaluation gives the same bits), and the per-sample
// arithmetic is the reference's unfused float
#pragma clang fp contract(off)

namespace {

using u64 = unsigned long long;
constexpr int kMom = 6;            // SI, SQ, SII, SQQ, SIQ, clips
constexpr int kMomThreads = 256;
constexpr int kMomVecs = 4;        // vectors per lane
// Samples of one block that a workgroup takes.  Its first vector may start up to kVec - 1 samples ahead of them (vectors
// are aligned in the caller's buffer, blocks are not), hence one vector less than the lanes can hold.
constexpr unsigned mom_chunk(bool s16) { return (kMomThreads * kMomVecs - 1) * (s16 ? 4 : 8); }
constexpr int kApplyThreads = 256;

struct ScanParams {
  double scale;     // (double)SCALE
  double n;         // block
  double dc_alpha;
  double rate;      // block / (adc_samprate * power_alpha)
  unsigned block;
};

__global__ void k_fe_init(kq_fe_status *state, u64 *mom) {
  if (threadIdx.x < kMom) mom[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    kq_fe_status s{};
    s.imbalance = 1.f;
    s.gain_i = s.gain_q = s.secphi = 1.f;
    *state = s;
  }
}

// Workgroup (x = row, y = chunk): the samples of the call that fall into chunk x of block `row`.  Every lane adds up its
// samples in integers, the lanes are reduced by shuffles and LDS, and six lanes issue one 64-bit atomic add each.
template <bool S16>
__global__ __launch_bounds__(kMomThreads) void k_fe_moments(const void *raw, unsigned n, unsigned off0, unsigned block,
                                                           u64 *mom) {
  constexpr int kVec = kq::fe_vec<S16>();
  constexpr unsigned kChunk = mom_chunk(S16);
  unsigned const row = blockIdx.x;
  // positions count from the start of row 0's block; the call's samples are [off0, off0 + n)
  u64 const lo64 = (u64)row * block + (u64)blockIdx.y * kChunk;
  u64 const hi64 = min(min(lo64 + kChunk, (u64)(row + 1) * block), (u64)off0 + n);
  u64 const lo = max(lo64, (u64)off0);
  long long acc[kMom] = {0, 0, 0, 0, 0, 0};
  if (lo < hi64) {
    unsigned const first = (unsigned)(lo - off0), last = (unsigned)(hi64 - off0);  // sample indices of the call
    unsigned const vb = first & ~(unsigned)(kVec - 1);
    auto add = [&](int i, int q) {
      if constexpr (!S16) {  // hackrf.c:146-153
        if (q == -128) {
          acc[5]++;
          q = -127;
        }
        if (i == -128) {
          acc[5]++;
          i = -127;
        }
      }
      acc[0] += i;
      acc[1] += q;
      acc[2] += i * i;
      acc[3] += q * q;
      acc[4] += i * q;
    };
#pragma unroll
    for (int k = 0; k < kMomVecs; k++) {
      unsigned const base = vb + (k * kMomThreads + threadIdx.x) * kVec;
      if (base >= last) continue;
      if (base >= first && base + kVec <= last) {
        uint4 const v = kq::fe_load_once(reinterpret_cast<const uint4 *>(raw) + base / kVec);
        unsigned const w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < kVec; j++) {
          if constexpr (S16)
            add((int)(short)(w[j] & 0xffff), (int)(short)(w[j] >> 16));
          else {
            unsigned const h = w[j >> 1] >> ((j & 1) * 16);
            add((int)(signed char)(h & 0xff), (int)(signed char)((h >> 8) & 0xff));
          }
        }
      } else {
        for (int j = 0; j < kVec; j++) {
          unsigned const idx = base + j;
          if (idx < first || idx >= last) continue;
          if constexpr (S16) {
            short2 const s = reinterpret_cast<const short2 *>(raw)[idx];
            add(s.x, s.y);
          } else {
            char2 const s = reinterpret_cast<const char2 *>(raw)[idx];
            add((int)(signed char)s.x, (int)(signed char)s.y);
          }
        }
      }
    }
  }
  __shared__ long long part[kMomThreads / 64][kMom];
#pragma unroll
  for (int m = 0; m < kMom; m++) {
    long long a = acc[m];
    for (int off = 32; off; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][m] = a;
  }
  __syncthreads();
  if (threadIdx.x < kMom) {
    long long a = 0;
    for (int w = 0; w < kMomThreads / 64; w++) a += part[w][threadIdx.x];
    if (a != 0) atomicAdd(mom + (size_t)row * kMom + threadIdx.x, (u64)a);  // two's complement: the signed sum
  }
}

__device__ __forceinline__ void write_row(float *table, unsigned row, const kq_fe_status &s) {
  float4 *p = reinterpret_cast<float4 *>(table + (size_t)row * kq::kFeRow);
  p[0] = make_float4(s.DC_i, s.DC_q, s.gain_i, s.gain_q);
  p[1] = make_float4(s.secphi, s.tanphi, 0.f, 0.f);
}

// One lane: the recursion of ka9q_hip.h over the call's completed blocks, from the carried state.  Row r of the table is
// what block r's samples are conditioned with, so row `completed` (the block left open) holds the final state.
__global__ void k_fe_scan(u64 *mom, unsigned completed, kq_fe_status *state, float *table, kq_fe_status *status_out,
                          ScanParams p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  kq_fe_status s = *state;
  double const S = p.scale, n = p.n, SS = S * S;
  for (unsigned r = 0; r < completed; r++) {
    write_row(table, r, s);
    const u64 *m = mom + (size_t)r * kMom;
    double const SI = (double)(long long)m[0], SQ = (double)(long long)m[1], SII = (double)(long long)m[2],
                 SQQ = (double)(long long)m[3], SIQ = (double)(long long)m[4];
    double const DC_i = s.DC_i, DC_q = s.DC_q, gain_i = s.gain_i, gain_q = s.gain_q;
    double const sI = S * SI, sQ = S * SQ;
    double const i_energy = SS * SII - 2.0 * DC_i * sI + n * (DC_i * DC_i);
    double const q_energy = SS * SQQ - 2.0 * DC_q * sQ + n * (DC_q * DC_q);
    double const cross = SS * SIQ - DC_q * sI - DC_i * sQ + n * (DC_i * DC_q);
    double const dotprod = (gain_i * gain_q) * cross;
    s.DC_i = (float)(DC_i + p.dc_alpha * (sI - n * DC_i));
    s.DC_q = (float)(DC_q + p.dc_alpha * (sQ - n * DC_q));
    double const block_energy = 0.5 * (i_energy + q_energy);
    if (block_energy > 0) {
      s.in_power = (float)(block_energy / n);
      double imbalance = s.imbalance, sinphi = s.sinphi;
      s.imbalance = (float)(imbalance + p.rate * (i_energy / q_energy - imbalance));
      double const dpn = dotprod / block_energy;
      s.sinphi = (float)(sinphi + p.rate * (dpn - sinphi));
      imbalance = s.imbalance;
      sinphi = s.sinphi;
      s.gain_q = (float)sqrt(0.5 * (1.0 + imbalance));
      s.gain_i = (float)sqrt(0.5 * (1.0 + 1.0 / imbalance));
      s.secphi = (float)(1.0 / sqrt(1.0 - sinphi * sinphi));
      s.tanphi = (float)((double)s.sinphi * (double)s.secphi);
    }
    s.samples += p.block;
    s.blocks += 1;
    s.clips += m[5];
    if (status_out) status_out[r] = s;
  }
  write_row(table, completed, s);
  *state = s;
  if (completed)  // the open block's moments move to row 0, where the next call's samples are added to them
    for (int k = 0; k < kMom; k++) mom[k] = mom[(size_t)completed * kMom + k];
}

__device__ __forceinline__ int16_t to_s16(float v) {
  // funcube.c:348 round(v * SHRT_MAX), saturated
  float const r = roundf(v * 32767.f);
  return (int16_t)(int)fminf(fmaxf(r, -32768.f), 32767.f);
}

// One lane per 16-byte vector of raw samples; the ragged end of the call sample by sample.
template <bool S16>
__global__ __launch_bounds__(kApplyThreads) void k_fe_apply(kq::FeRaw r, unsigned n, float2 *out, int16_t *out16) {
  constexpr int kVec = kq::fe_vec<S16>();
  unsigned const base = (blockIdx.x * kApplyThreads + threadIdx.x) * kVec;
  if (base >= n) return;
  auto put = [&](unsigned idx, float2 w0, float2 w1) {
    if (out) *reinterpret_cast<float4 *>(out + idx) = make_float4(w0.x, w0.y, w1.x, w1.y);
    if (out16) {
      short4 q;
      q.x = to_s16(w0.x);
      q.y = to_s16(w0.y);
      q.z = to_s16(w1.x);
      q.w = to_s16(w1.y);
      *reinterpret_cast<short4 *>(out16 + 2 * (size_t)idx) = q;
    }
  };
  if (base + kVec <= n) {
    uint4 const v = kq::fe_load_once(reinterpret_cast<const uint4 *>(r.raw) + base / kVec);
    kq::fe_vector<S16>(r, v, kq::fe_locate(r, base), [&](int j, float2 w0, float2 w1) { put(base + j, w0, w1); });
  } else {
    for (unsigned idx = base; idx < n; idx++) {
      float2 const w = kq::fe_sample<S16>(r, idx);
      if (out) out[idx] = w;
      if (out16) *reinterpret_cast<short2 *>(out16 + 2 * (size_t)idx) = make_short2(to_s16(w.x), to_s16(w.y));
    }
  }
}

}  // namespace

struct kq_frontend : kq::HostSide {
  kq_fe_config cfg;
  ScanParams scan;
  unsigned filled = 0;          // samples of the open block seen so far
  size_t max_rows = 0;          // rows of `mom`, `table`, `status_dev`
  u64 *mom = nullptr;           // [max_rows][kMom]; row 0 carries the open block between calls
  float *table = nullptr;       // [max_rows][kFeRow]
  kq_fe_status *state = nullptr;
  // staging of host-memory calls
  void *raw_dev = nullptr;
  float2 *cf_dev = nullptr;
  int16_t *s16_dev = nullptr;
  float *energy_dev = nullptr;
  kq_fe_status *status_dev = nullptr;
};

static size_t fe_bytes_per_sample(const kq_frontend *fe) { return fe->cfg.format == KQ_FE_S16 ? 4 : 2; }

static int fe_alloc(kq_frontend *fe) {
  kq::DeviceScope dev_scope_(fe->cfg.device);
  if (fe->open_stream(fe->cfg.stream)) return -1;
  fe->max_rows = fe->cfg.max_samples / fe->cfg.block + 3;
  if (fe->alloc(&fe->mom, fe->max_rows * kMom) || fe->alloc(&fe->table, fe->max_rows * kq::kFeRow) ||
      fe->alloc(&fe->state, 1))
    return -1;
  hipLaunchKernelGGL(k_fe_init, dim3(1), dim3(64), 0, fe->stream, fe->state, fe->mom);
  KQ_TRY(hipGetLastError());
  KQ_TRY(hipStreamSynchronize(fe->stream));
  return 0;
}

static int fe_staging(kq_frontend *fe) {
  if (fe->raw_dev) return 0;
  size_t const n = fe->cfg.max_samples;
  char *raw = nullptr;
  if (fe->alloc(&raw, n * fe_bytes_per_sample(fe) + 16) || fe->alloc(&fe->cf_dev, n) || fe->alloc(&fe->s16_dev, 2 * n) ||
      fe->alloc(&fe->energy_dev, 1) || fe->alloc(&fe->status_dev, fe->max_rows))
    return -1;
  fe->raw_dev = raw;
  return 0;
}

// moments and scan of a call of n samples at `raw` (device memory); `what` fills in the table description the kernels
// behind it need and *completed the number of blocks that end inside the call
static int fe_estimate(kq_frontend *fe, const void *raw, size_t n, kq_fe_status *status_dev, kq::FeRaw *what,
                       unsigned *completed) {
  unsigned const block = fe->cfg.block, off0 = fe->filled;
  bool const s16 = fe->cfg.format == KQ_FE_S16;
  unsigned const rows = (unsigned)(((size_t)off0 + n + block - 1) / block);
  *completed = (unsigned)(((size_t)off0 + n) / block);
  KQ_TRY(hipMemsetAsync(fe->mom + kMom, 0, sizeof(u64) * kMom * (size_t)rows, fe->stream));
  unsigned const chunk = mom_chunk(s16);
  dim3 const grid(rows, (unsigned)((std::min((size_t)block, (size_t)off0 + n) + chunk - 1) / chunk));
  if (s16)
    hipLaunchKernelGGL(k_fe_moments<true>, grid, dim3(kMomThreads), 0, fe->stream, raw, (unsigned)n, off0, block, fe->mom);
  else
    hipLaunchKernelGGL(k_fe_moments<false>, grid, dim3(kMomThreads), 0, fe->stream, raw, (unsigned)n, off0, block, fe->mom);
  hipLaunchKernelGGL(k_fe_scan, dim3(1), dim3(64), 0, fe->stream, fe->mom, *completed, fe->state, fe->table, status_dev,
                     fe->scan);
  KQ_TRY(hipGetLastError());
  *what = kq::FeRaw{raw, fe->table, block, off0, s16 ? 1 : 0};
  fe->filled = (unsigned)(((size_t)off0 + n) % block);
  return 0;
}

static int fe_check_call(const char *fn, kq_frontend *fe, const void *raw, int on_device, size_t n) {
  if (!fe || !raw) {
    kq_internal_set_error("%s: null argument", fn);
    return -1;
  }
  if (n > fe->cfg.max_samples) {
    kq_internal_set_error("%s: %zu samples exceed max_samples %zu", fn, n, fe->cfg.max_samples);
    return -1;
  }
  if (on_device && ((uintptr_t)raw & 15)) {
    kq_internal_set_error("%s: raw samples in device memory must be 16-byte aligned", fn);
    return -1;
  }
  return 0;
}

extern "C" {

kq_frontend *kq_fe_create(const kq_fe_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_fe_create: null config");
    return nullptr;
  }
  if (cfg->format != KQ_FE_S8 && cfg->format != KQ_FE_S16) {
    kq_internal_set_error("kq_fe_create: format must be KQ_FE_S8 or KQ_FE_S16");
    return nullptr;
  }
  if (cfg->block < 64 || cfg->block > (1u << 22)) {
    kq_internal_set_error("kq_fe_create: block must be 64 .. 4194304 samples");
    return nullptr;
  }
  if (!(cfg->adc_samprate > 0) || !(cfg->dc_alpha > 0) || !(cfg->power_alpha > 0)) {
    kq_internal_set_error("kq_fe_create: adc_samprate, dc_alpha and power_alpha must be positive");
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 31)) {
    kq_internal_set_error("kq_fe_create: max_samples must be 1 .. 2^31");
    return nullptr;
  }
  kq_frontend *fe = new kq_frontend;
  fe->cfg = *cfg;
  bool const s16 = cfg->format == KQ_FE_S16;
  fe->scan.scale = s16 ? (double)(float)(1. / 32767.) : (double)(float)(1. / 127.);
  fe->scan.n = (double)cfg->block;
  fe->scan.dc_alpha = cfg->dc_alpha;
  fe->scan.rate = (double)cfg->block / (cfg->adc_samprate * cfg->power_alpha);
  fe->scan.block = cfg->block;
  if (fe_alloc(fe) != 0) {
    kq_fe_destroy(fe);
    return nullptr;
  }
  return fe;
}

int kq_fe_destroy(kq_frontend *fe) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (!fe) return -1;
  fe->close();
  delete fe;
  return 0;
}

int kq_fe_reset(kq_frontend *fe) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (!fe) return -1;
  hipLaunchKernelGGL(k_fe_init, dim3(1), dim3(64), 0, fe->stream, fe->state, fe->mom);
  KQ_TRY(hipGetLastError());
  fe->filled = 0;
  return 0;
}

int kq_fe_sync(kq_frontend *fe) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (!fe) return -1;
  KQ_TRY(hipStreamSynchronize(fe->stream));
  return 0;
}

void *kq_fe_stream(kq_frontend *fe) { return fe ? (void *)fe->stream : nullptr; }

int kq_fe_process(kq_frontend *fe, const void *raw, int on_device, size_t n, float *out_cf32, int16_t *out_s16,
                  kq_fe_status *block_status) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (fe_check_call("kq_fe_process", fe, raw, on_device, n)) return -1;
  if (n == 0) return 0;
  float2 *cf = (float2 *)out_cf32;
  int16_t *s16 = out_s16;
  kq_fe_status *st = block_status;
  if (!on_device) {
    if (fe_staging(fe)) return -1;
    KQ_TRY(hipMemcpyAsync(fe->raw_dev, raw, n * fe_bytes_per_sample(fe), hipMemcpyHostToDevice, fe->stream));
    raw = fe->raw_dev;
    cf = out_cf32 ? fe->cf_dev : nullptr;
    s16 = out_s16 ? fe->s16_dev : nullptr;
    st = block_status ? fe->status_dev : nullptr;
  }
  kq::FeRaw what;
  unsigned completed = 0;
  if (fe_estimate(fe, raw, n, st, &what, &completed)) return -1;
  if (cf || s16) {
    unsigned const per = kApplyThreads * (what.s16 ? 4 : 8);
    dim3 const grid((unsigned)((n + per - 1) / per));
    if (what.s16)
      hipLaunchKernelGGL(k_fe_apply<true>, grid, dim3(kApplyThreads), 0, fe->stream, what, (unsigned)n, cf, s16);
    else
      hipLaunchKernelGGL(k_fe_apply<false>, grid, dim3(kApplyThreads), 0, fe->stream, what, (unsigned)n, cf, s16);
    KQ_TRY(hipGetLastError());
  }
  if (!on_device) {
    if (out_cf32) KQ_TRY(hipMemcpyAsync(out_cf32, cf, sizeof(float2) * n, hipMemcpyDeviceToHost, fe->stream));
    if (out_s16) KQ_TRY(hipMemcpyAsync(out_s16, s16, sizeof(int16_t) * 2 * n, hipMemcpyDeviceToHost, fe->stream));
    if (block_status && completed)
      KQ_TRY(hipMemcpyAsync(block_status, st, sizeof(kq_fe_status) * completed, hipMemcpyDeviceToHost, fe->stream));
    KQ_TRY(hipStreamSynchronize(fe->stream));
  }
  return (int)completed;
}

int kq_fe_process_decim(kq_frontend *fe, kq_decimator *dec, const void *raw, int on_device, size_t n_out, float *out_cf32,
                        int16_t *out_s16, float *out_energy, kq_fe_status *block_status) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (!dec || !out_cf32) {
    kq_internal_set_error("kq_fe_process_decim: null argument");
    return -1;
  }
  kq_decim_internal_info di;
  kq_decim_internal_get_info(dec, &di);
  size_t const n = n_out << di.log_decimate;
  if (fe_check_call("kq_fe_process_decim", fe, raw, on_device, n)) return -1;
  if (di.device != fe->cfg.device || di.stream != (void *)fe->stream) {
    kq_internal_set_error("kq_fe_process_decim: the front end and the decimator must be on the same device and stream "
                          "(kq_fe_stream gives the stream for kq_decim_config)");
    return -1;
  }
  if (n_out > di.max_out) {
    kq_internal_set_error("kq_fe_process_decim: n_out %zu exceeds the decimator's max_out %zu", n_out, di.max_out);
    return -1;
  }
  if (n_out == 0) return 0;
  float *cf = out_cf32, *energy = out_energy;
  int16_t *s16 = out_s16;
  kq_fe_status *st = block_status;
  if (!on_device) {
    if (fe_staging(fe)) return -1;
    KQ_TRY(hipMemcpyAsync(fe->raw_dev, raw, n * fe_bytes_per_sample(fe), hipMemcpyHostToDevice, fe->stream));
    raw = fe->raw_dev;
    cf = (float *)fe->cf_dev;
    s16 = out_s16 ? fe->s16_dev : nullptr;
    energy = out_energy ? fe->energy_dev : nullptr;
    st = block_status ? fe->status_dev : nullptr;
  }
  kq::FeRaw what;
  unsigned completed = 0;
  if (fe_estimate(fe, raw, n, st, &what, &completed)) return -1;
  if (kq_decim_internal_process_raw(dec, what, n_out, cf, s16, energy)) return -1;
  if (!on_device) {
    KQ_TRY(hipMemcpyAsync(out_cf32, cf, sizeof(float2) * n_out, hipMemcpyDeviceToHost, fe->stream));
    if (out_s16) KQ_TRY(hipMemcpyAsync(out_s16, s16, sizeof(int16_t) * 2 * n_out, hipMemcpyDeviceToHost, fe->stream));
    if (out_energy) KQ_TRY(hipMemcpyAsync(out_energy, energy, sizeof(float), hipMemcpyDeviceToHost, fe->stream));
    if (block_status && completed)
      KQ_TRY(hipMemcpyAsync(block_status, st, sizeof(kq_fe_status) * completed, hipMemcpyDeviceToHost, fe->stream));
    if (kq_decim_sync(dec)) return -1;  // the same stream; also reports an output energy that never arrived
  }
  return (int)completed;
}

int kq_fe_get_status(kq_frontend *fe, kq_fe_status *out) {
  kq::DeviceScope dev_scope_(fe ? fe->cfg.device : -1);
  if (!fe || !out) return -1;
  KQ_TRY(hipMemcpyAsync(out, fe->state, sizeof(kq_fe_status), hipMemcpyDeviceToHost, fe->stream));
  KQ_TRY(hipStreamSynchronize(fe->stream));
  return 0;
}

}  // extern "C"
