// kq_rsmp.hip -- rational resampler bank: thousands of PCM rows from Fi = in_rate_num / in_rate_den to Fo = out_rate on
// gfx950, a polyphase Kaiser-windowed sinc.
//
// The definition is in include/ka9q_hip.h (kq_rsmp_*): output j reads the T inputs ending at n_j = floor(j Q / P) through
// row phi_j = (j Q) mod P of g, folded by fmaf from 0.0f in tap order.  n and j are 64-bit and lie on one grid for every
// slot, so J, the outputs of a call, is known on the host.  The host keeps every slot's settings and uploads the table
// when one changed (kq_rsmp_set and kq_rsmp_remove touch no device); a slot's input is zero before RsmpPar::n_set, so a
// set or a reset costs the device nothing.  Carried per slot and side: the last T - 1 inputs as floats, two copies
// written in turn (a call's tiles read one while its first tile writes the other).
//
// k_rsmp  one workgroup per (active slot, tile of `tile` outputs): the tile's input span -- carried samples, then the
//         call's, gathered block by block, int16 words converted -- into LDS, both sides of a stereo slot; then one
//         output per lane and pass.  The coefficients are read from global memory as gt[k][j mod P] = g[phi_j][k]: the
//         rows in the order the outputs visit them, so neighbouring lanes read neighbouring words (P = 1: one word for
//         the whole wave, a scalar load).  The table is at most 1 MiB and stays in L2.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_lane.hpp"
#include "kq_slots.hpp"

namespace {

constexpr unsigned kMaxSlots = 65536;
constexpr unsigned kMaxP = 4096, kMinT = 4, kMaxT = 256, kMaxTable = 1u << 18;
constexpr int kThreads = 256;
constexpr unsigned kTileMax = 1024;  // outputs per workgroup at most
constexpr unsigned kSpan = 4096;     // input samples per side a workgroup stages: 32 KiB of LDS, five workgroups per CU
constexpr unsigned kTilesPerLaunch = 32768;
constexpr float kScale = 1.f / SHRT_MAX;

struct RsmpPar {  // per slot, as the kernel reads it
  int active;
  unsigned source;
  int channels;
  int pad;
  long long n_set;  // the sample the slot was set at: zero input before it
};

struct RsmpCall {
  const RsmpPar *par;
  const int *list;        // active slots, ascending
  const int *rowmap;      // per list entry: the row of `src` (host input, staged) or null (par.source)
  const float *gt;        // [T][P]: gt[k P + r] = g[(r Q) mod P][k]
  const float *hist_in;   // [S][2][T - 1]: x[n0 - (T - 1) .. n0 - 1] per side
  float *hist_out;        // the same for n1
  long long n0, n1;       // the call's samples
  long long j0, J;        // its first output and their number
  unsigned P, Q, T, tile;
  const void *src;
  size_t src_stride, row_stride;
  unsigned block_len;
  float *out;
  size_t out_stride;
  int16_t *pcm;
  size_t pcm_stride;
};

// side c of the call's m-th sample of a slot with ch sides
template <int FORMAT>
__device__ __forceinline__ float rsmp_sample(RsmpCall const &a, size_t base, unsigned ch, unsigned m, unsigned c) {
  unsigned const k = m / a.block_len, i = m - k * a.block_len;
  size_t const e = base + (size_t)k * a.row_stride + (size_t)i * ch + c;
  if constexpr (FORMAT == KQ_PCM_S16BE) {
    unsigned const w = reinterpret_cast<const unsigned short *>(a.src)[e];
    short const s = (short)(((w << 8) | (w >> 8)) & 0xffffu);  // ntohs
    return __fmul_rn(kScale, (float)s);
  } else {
    return reinterpret_cast<const float *>(a.src)[e];
  }
}

// grid (active slots, tiles of this launch); tile0: the launch's first tile
template <int FORMAT, bool P1>
__global__ __launch_bounds__(kThreads) void k_rsmp(RsmpCall a, unsigned tile0) {
  __shared__ float xs[2][kSpan];
  unsigned const li = blockIdx.x, tile = tile0 + blockIdx.y, tid = threadIdx.x;
  int const slot = a.list[li];
  RsmpPar const p = a.par[slot];
  size_t const row = a.rowmap ? (size_t)a.rowmap[li] : (size_t)p.source;
  size_t const base = row * a.src_stride;
  unsigned const ch = p.channels == 2 ? 2u : 1u, T = a.T, H = T - 1, P = P1 ? 1u : a.P, Q = a.Q;
  const float *hin = a.hist_in + (size_t)slot * 2 * H;
  // x[n] of side c: zero before the slot was set, carried before the call, else the call's
  auto fetch = [&](long long n, unsigned c) -> float {
    if (n < p.n_set) return 0.f;
    if (n < a.n0) return hin[c * H + H - (unsigned)(a.n0 - n)];
    return rsmp_sample<FORMAT>(a, base, ch, (unsigned)(n - a.n0), c);
  };
  long long const jt = (long long)tile * a.tile;  // the tile's first output, counted from the call's
  long long const left = a.J - jt;
  unsigned const nj = left <= 0 ? 0u : (left < (long long)a.tile ? (unsigned)left : a.tile);
  unsigned long long const jq = (unsigned long long)(a.j0 + jt) * Q;
  long long const nb = (long long)(jq / P);  // n of the tile's first output
  unsigned const rb = (unsigned)(jq % P), r0 = (unsigned)((unsigned long long)(a.j0 + jt) % P);
  if (nj) {
    // xs[c][i] = x[nb - (T - 1) + i] up to the last output's n; at most kSpan by the host's choice of `tile`
    unsigned const span = (rb + (nj - 1) * Q) / P + T;
    long long const ns = nb - (long long)H;
    for (unsigned i = tid; i < span; i += kThreads)
      for (unsigned c = 0; c < ch; c++) xs[c][i] = fetch(ns + i, c);
  }
  if (tile == 0) {  // the next call's carried samples (the other copy: the tiles of this call still read this one)
    float *hout = a.hist_out + (size_t)slot * 2 * H;
    unsigned long long const ncall = (unsigned long long)(a.n1 - a.n0);
    for (unsigned i = tid; i < H; i += kThreads) {
      long long const n = a.n1 - (long long)H + i;
      for (unsigned c = 0; c < ch; c++)
        hout[c * H + i] = n < a.n0 ? hin[c * H + i + ncall] : rsmp_sample<FORMAT>(a, base, ch, (unsigned)(n - a.n0), c);
    }
  }
  __syncthreads();
  for (unsigned q = tid; q < nj; q += kThreads) {
    unsigned const at = (rb + q * Q) / P + H;  // x[n_j] in xs
    const float *g = a.gt + (P1 ? 0u : (r0 + q) % P);
    size_t const jc = (size_t)(jt + q) * ch;
    float l = 0.f, r = 0.f;
    if (ch == 2) {
#pragma unroll 4
      for (unsigned k = 0; k < T; k++) {
        float const c = g[(size_t)k * P];
        l = __fmaf_rn(c, xs[0][at - k], l);
        r = __fmaf_rn(c, xs[1][at - k], r);
      }
    } else {
#pragma unroll 4
      for (unsigned k = 0; k < T; k++) l = __fmaf_rn(g[(size_t)k * P], xs[0][at - k], l);
    }
    if (a.out) {
      float *o = a.out + (size_t)slot * a.out_stride + jc;
      o[0] = l;
      if (ch == 2) o[1] = r;
    }
    if (a.pcm) {
      int16_t *o = a.pcm + (size_t)slot * a.pcm_stride + jc;
      o[0] = (int16_t)kq::pcm_word_be(l);
      if (ch == 2) o[1] = (int16_t)kq::pcm_word_be(r);
    }
  }
}

unsigned long long ceil_mul_div(unsigned long long n, unsigned P, unsigned Q) {  // ceil(n P / Q) without overflow
  return (unsigned long long)(((unsigned __int128)n * P + (Q - 1)) / Q);
}

// g[phi][k] = (float)h[k P + phi], h the Kaiser-windowed sinc of K = P T taps at rate P Fi in double, sum h = P
std::vector<float> design(unsigned P, unsigned T, double Fi, double cutoff, double beta) {
  size_t const K = (size_t)P * T;
  std::vector<double> h(K);
  double const den = kq::i0_double(M_PI * beta), c = 0.5 * (double)(K - 1);
  double sum = 0;
  for (size_t m = 0; m < K; m++) {
    double const pp = 2.0 * (double)m / (double)(K - 1) - 1.0;  // make_kaiser, filter.c:337-357
    double const w = kq::i0_double(M_PI * beta * std::sqrt(std::max(0.0, 1.0 - pp * pp))) / den;
    double const t = 2.0 * cutoff / ((double)P * Fi) * ((double)m - c);
    h[m] = (t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t)) * w;
    sum += h[m];
  }
  std::vector<float> g(K);
  for (unsigned phi = 0; phi < P; phi++)
    for (unsigned k = 0; k < T; k++) g[(size_t)phi * T + k] = (float)(h[(size_t)k * P + phi] * (double)P / sum);
  return g;
}

}  // namespace

struct kq_rsmp_bank : kq::HostSide {
  kq_rsmp_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  unsigned P = 0, Q = 0, T = 0, tile = 0;
  uint64_t n_cur = 0, j_cur = 0;  // j_cur = ceil(n_cur P / Q)
  int turn = 0;                   // the copy of the carried samples the next call reads
  std::vector<float> g;           // [P][T]
  std::vector<RsmpPar> want;      // [max_slots] the slots as set; d.slots follows at the next call
  bool dirty = false;
  unsigned nset = 0, nstereo = 0; // slots set; the stereo ones among them
  struct Dev {  // kq::lazy_device
    kq::SlotTable<RsmpPar> slots;
    float *gt = nullptr;
    float *hist[2] = {nullptr, nullptr};
    // host-memory calls
    float *out = nullptr;
    size_t out_cap = 0;
    int16_t *pcm = nullptr;
    size_t pcm_cap = 0;
  } d;
};

namespace {

int make_device(kq_rsmp_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots, H = b->T - 1, K = b->g.size();
  if (d.slots.alloc(*b, S) || b->alloc(&d.gt, K) || b->alloc(&d.hist[0], S * 2 * H, true) || b->alloc(&d.hist[1], S * 2 * H, true))
    return -1;
  std::vector<float> gt(K);  // the rows in the order the outputs visit them, tap-major
  for (unsigned r = 0; r < b->P; r++) {
    unsigned const phi = (unsigned)(((unsigned long long)r * b->Q) % b->P);
    for (unsigned k = 0; k < b->T; k++) gt[(size_t)k * b->P + r] = b->g[(size_t)phi * b->T + k];
  }
  KQ_TRY(hipMemcpyAsync(d.gt, gt.data(), K * sizeof(float), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// the slot table from `want`, and its upload on the stream; waits, before (earlier calls read the table) and after (the
// host copies may change again)
int flush(kq_rsmp_bank *b) {
  auto &t = b->d.slots;
  KQ_TRY(hipStreamSynchronize(b->stream));
  t.par = b->want;
  t.all.clear();
  for (size_t k = 0; k < t.par.size(); k++)
    if (t.par[k].active) t.all.push_back((int)k);
  KQ_TRY(hipMemcpyAsync(t.d_par, t.par.data(), t.par.size() * sizeof(RsmpPar), hipMemcpyHostToDevice, b->stream));
  if (!t.all.empty()) KQ_TRY(hipMemcpyAsync(t.d_list, t.all.data(), t.all.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  b->dirty = false;
  return 0;
}

}  // namespace

extern "C" {

kq_rsmp_bank *kq_rsmp_create(const kq_rsmp_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_rsmp_create: null config");
    return nullptr;
  }
  if (cfg->in_rate_num <= 0 || cfg->in_rate_den <= 0) {
    kq_internal_set_error("kq_rsmp_create: in_rate_num %d and in_rate_den %d must be positive", cfg->in_rate_num, cfg->in_rate_den);
    return nullptr;
  }
  long long const num = cfg->in_rate_num, den = cfg->in_rate_den;
  if (num < 8000 * den || num > 384000 * den) {
    kq_internal_set_error("kq_rsmp_create: in_rate_num %d / in_rate_den %d must be 8000..384000 Hz", cfg->in_rate_num,
                          cfg->in_rate_den);
    return nullptr;
  }
  if (cfg->out_rate < 8000 || cfg->out_rate > 384000) {
    kq_internal_set_error("kq_rsmp_create: out_rate %d must be 8000..384000", cfg->out_rate);
    return nullptr;
  }
  long long p = (long long)cfg->out_rate * den, q = num;
  long long const gcd = std::gcd(p, q);
  p /= gcd;
  q /= gcd;
  if (16 * p < q || p > 16 * q) {
    kq_internal_set_error("kq_rsmp_create: out_rate %d over in_rate_num %d / in_rate_den %d is P / Q = %lld / %lld, must be 1/16..16",
                          cfg->out_rate, cfg->in_rate_num, cfg->in_rate_den, p, q);
    return nullptr;
  }
  if (p > kMaxP) {
    kq_internal_set_error("kq_rsmp_create: out_rate %d over in_rate_num %d / in_rate_den %d gives P = %lld phases, %u at most",
                          cfg->out_rate, cfg->in_rate_num, cfg->in_rate_den, p, kMaxP);
    return nullptr;
  }
  unsigned const T = cfg->taps;
  if (T < kMinT || T > kMaxT) {
    kq_internal_set_error("kq_rsmp_create: taps %u must be %u..%u", T, kMinT, kMaxT);
    return nullptr;
  }
  if ((unsigned long long)p * T > kMaxTable) {
    kq_internal_set_error("kq_rsmp_create: taps %u x P %lld = %llu coefficients, 2^18 at most", T, p, (unsigned long long)p * T);
    return nullptr;
  }
  double const Fi = (double)num / (double)den, edge = 0.5 * std::min(Fi, (double)cfg->out_rate);
  if (!(cfg->cutoff_hz > 0) || !((double)cfg->cutoff_hz < edge)) {
    kq_internal_set_error("kq_rsmp_create: cutoff_hz %g must be above 0 and below min(Fi, Fo) / 2 = %g", (double)cfg->cutoff_hz, edge);
    return nullptr;
  }
  if (!std::isfinite(cfg->kaiser_beta) || cfg->kaiser_beta < 0) {
    kq_internal_set_error("kq_rsmp_create: kaiser_beta must be finite and >= 0");
    return nullptr;
  }
  if (cfg->max_slots == 0 || cfg->max_slots > kMaxSlots) {
    kq_internal_set_error("kq_rsmp_create: max_slots %u must be 1..%u", cfg->max_slots, kMaxSlots);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_rsmp_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  kq_rsmp_bank *b = new kq_rsmp_bank;
  b->cfg = *cfg;
  b->P = (unsigned)p;
  b->Q = (unsigned)q;
  b->T = T;
  // the span of a tile is below (tile - 1) Q / P + 1 + T samples
  b->tile = (unsigned)std::min<unsigned long long>(kTileMax, 1 + (unsigned long long)(kSpan - T - 1) * b->P / b->Q);
  b->g = design(b->P, T, Fi, cfg->cutoff_hz, cfg->kaiser_beta);
  b->want.assign(cfg->max_slots, RsmpPar{});
  return b;
}

int kq_rsmp_destroy(kq_rsmp_bank *b) { return kq::destroy_bank(b, "kq_rsmp_destroy"); }

int kq_rsmp_set(kq_rsmp_bank *b, unsigned slot, const kq_rsmp_params *p) {
  if (!kq::set_args_ok("kq_rsmp_set", slot, p, kMaxSlots)) return -1;
  if (p->channels != 1 && p->channels != 2) {
    kq_internal_set_error("kq_rsmp_set: channels %d must be 1 or 2", p->channels);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_rsmp_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("kq_rsmp_set", slot, b->cfg.max_slots)) return -1;
  RsmpPar &w = b->want[slot];
  if (w.active && w.channels == 2) b->nstereo--;
  if (!w.active) b->nset++;
  w = RsmpPar{};
  w.active = 1;
  w.source = p->source;
  w.channels = p->channels;
  w.n_set = (long long)b->n_cur;
  if (p->channels == 2) b->nstereo++;
  b->dirty = true;
  return 0;
}

int kq_rsmp_remove(kq_rsmp_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_remove: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots || !b->want[slot].active) {
    kq_internal_set_error("kq_rsmp_remove: slot %u holds no resampler", slot);
    return -1;
  }
  if (b->want[slot].channels == 2) b->nstereo--;
  b->nset--;
  b->want[slot] = RsmpPar{};
  b->dirty = true;
  return 0;
}

size_t kq_rsmp_max_out(const kq_rsmp_bank *b, size_t nsamples) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_max_out: null bank");
    return 0;
  }
  return (size_t)ceil_mul_div(nsamples, b->P, b->Q);
}

int kq_rsmp_get_info(kq_rsmp_bank *b, kq_rsmp_info *info) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_get_info: null bank");
    return -1;
  }
  if (!info) {
    kq_internal_set_error("kq_rsmp_get_info: null info");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  info->P = b->P;
  info->Q = b->Q;
  info->taps = b->T;
  info->delay_in_samples = ((double)b->P * b->T - 1.0) / (2.0 * b->P);
  info->next_in = b->n_cur;
  info->next_out = b->j_cur;
  return 0;
}

int kq_rsmp_get_taps(const kq_rsmp_bank *b, float *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_get_taps: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_rsmp_get_taps: null dst");
    return -1;
  }
  size_t const n = std::min(cap, b->g.size());
  if (n) std::memcpy(dst, b->g.data(), n * sizeof(float));
  return (int)b->g.size();
}

int kq_rsmp_process(kq_rsmp_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, float *out, size_t out_stride, int16_t *pcm, size_t pcm_stride) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_process: null bank");
    return -1;
  }
  if (format != KQ_PCM_F32 && format != KQ_PCM_S16BE) {
    kq_internal_set_error("kq_rsmp_process: unknown sample format %d", format);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_rsmp_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  unsigned const cmax = b->nstereo ? 2u : 1u;
  if (nblocks > 1 && row_stride < (size_t)cmax * block_len) {
    kq_internal_set_error("kq_rsmp_process: row_stride %zu < %zu, a block of block_len %u samples of a stereo slot", row_stride,
                          (size_t)cmax * block_len, block_len);
    return -1;
  }
  uint64_t const j1 = ceil_mul_div(b->n_cur + ncall, b->P, b->Q), J = j1 - b->j_cur;
  if (J > (uint64_t)INT_MAX) {
    kq_internal_set_error("kq_rsmp_process: nblocks %u x block_len %u gives J = %llu outputs, beyond what the return value holds",
                          nblocks, block_len, (unsigned long long)J);
    return -1;
  }
  if (out && out_stride < cmax * J) {
    kq_internal_set_error("kq_rsmp_process: out_stride %zu < %u J = %llu", out_stride, cmax, (unsigned long long)(cmax * J));
    return -1;
  }
  if (pcm && pcm_stride < cmax * J) {
    kq_internal_set_error("kq_rsmp_process: pcm_stride %zu < %u J = %llu", pcm_stride, cmax, (unsigned long long)(cmax * J));
    return -1;
  }
  if (ncall == 0) return 0;
  if (!src) {
    kq_internal_set_error("kq_rsmp_process: null src");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (b->dirty && (b->dev_ready || b->nset)) {  // (a bank nobody has set a slot of stays without a device)
    if (kq::lazy_device(b, make_device) || flush(b)) return -1;
  }
  kq::CallWork const work = kq::call_work(b, "kq_rsmp_process", ncall, src, "src");
  if (work == kq::CALL_IDLE) {
    b->n_cur += ncall;
    b->j_cur = j1;
    return (int)J;
  }
  if (work != kq::CALL_RUN) return work;
  auto &d = b->d;
  size_t const nlist = d.slots.all.size(), rows = (size_t)d.slots.all.back() + 1;
  RsmpCall a{};
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.gt = d.gt;
  a.hist_in = d.hist[b->turn];
  a.hist_out = d.hist[b->turn ^ 1];
  a.n0 = (long long)b->n_cur;
  a.n1 = a.n0 + (long long)ncall;
  a.j0 = (long long)b->j_cur;
  a.J = (long long)J;
  a.P = b->P;
  a.Q = b->Q;
  a.T = b->T;
  a.tile = b->tile;
  a.block_len = block_len;
  if (on_device) {
    a.src = src;
    a.src_stride = src_stride;
    a.row_stride = nblocks > 1 ? row_stride : 0;
    a.rowmap = nullptr;
    a.out = out;
    a.out_stride = out_stride;
    a.pcm = pcm;
    a.pcm_stride = pcm_stride;
  } else {
    // (the stage is sized by the call, not by max_samples: it only ever grows)
    kq::Staged in;
    if (d.slots.stage_rows(*b, src, format == KQ_PCM_S16BE ? 2 : 4, src_stride, row_stride, block_len, nblocks,
                           ncall * cmax * 4, &in, cmax, [](RsmpPar const &p) { return (unsigned)p.channels; }))
      return -1;
    a.src = in.src;
    a.src_stride = in.src_stride;
    a.row_stride = in.row_stride;
    a.rowmap = in.rowmap;
    // the outputs as planes of their own, a row per slot up to the last active one
    if (out && J && b->grow(&d.out, &d.out_cap, rows * cmax * J)) return -1;
    if (pcm && J && b->grow(&d.pcm, &d.pcm_cap, rows * cmax * J)) return -1;
    a.out = out && J ? d.out : nullptr;
    a.pcm = pcm && J ? d.pcm : nullptr;
    a.out_stride = a.pcm_stride = cmax * J;
  }
  auto const kern = format == KQ_PCM_S16BE ? (b->P == 1 ? k_rsmp<KQ_PCM_S16BE, true> : k_rsmp<KQ_PCM_S16BE, false>)
                                           : (b->P == 1 ? k_rsmp<KQ_PCM_F32, true> : k_rsmp<KQ_PCM_F32, false>);
  // (a call without outputs still runs its first tile: it carries the samples on)
  uint64_t const tiles = std::max<uint64_t>(1, (J + b->tile - 1) / b->tile);
  for (uint64_t t0 = 0; t0 < tiles; t0 += kTilesPerLaunch) {
    unsigned const nt = (unsigned)std::min<uint64_t>(kTilesPerLaunch, tiles - t0);
    hipLaunchKernelGGL(kern, dim3((unsigned)nlist, nt), dim3(kThreads), 0, b->stream, a, (unsigned)t0);
    KQ_TRY(hipGetLastError());
  }
  b->turn ^= 1;  // from here on the carried samples are in the other copy, whatever fails below
  b->n_cur += ncall;
  b->j_cur = j1;
  if (!on_device) {
    // the rows of the active slots, as far as each slot wrote: runs of neighbours with the same number of sides
    auto const &all = d.slots.all;
    auto const &par = d.slots.par;
    for (size_t i = 0; i < all.size() && J;) {
      size_t k = i + 1;
      while (k < all.size() && all[k] == all[k - 1] + 1 && par[all[k]].channels == par[all[i]].channels) k++;
      size_t const w = (size_t)par[all[i]].channels * J;
      if (out && kq::copy_rows_back(*b, out, out_stride, d.out, a.out_stride, w, sizeof(float), (size_t)all[i], k - i)) return -1;
      if (pcm && kq::copy_rows_back(*b, pcm, pcm_stride, d.pcm, a.pcm_stride, w, sizeof(int16_t), (size_t)all[i], k - i)) return -1;
      i = k;
    }
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  return (int)J;
}

int kq_rsmp_sync(kq_rsmp_bank *b) { return kq::sync_bank(b, "kq_rsmp_sync"); }

int kq_rsmp_reset(kq_rsmp_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_rsmp_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = b->j_cur = 0;
  for (RsmpPar &w : b->want) w.n_set = 0;  // nothing carried is valid: no device work
  b->dirty = true;
  return 0;
}

}  // extern "C"
