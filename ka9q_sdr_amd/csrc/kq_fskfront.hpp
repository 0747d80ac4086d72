// kq_fskfront.hpp -- the front end that the baseband FSK banks share (kq_fsk: HDLC packet and AIS; kq_pag: POCSAG): flat FM
// discriminator output -> one decision per sample, packed 64 to a word, and the shift DPLL that takes a channel bit per
// symbol.  The algorithm is the header's (include/ka9q_hip.h, kq_fsk_*: quantise, low-pass, threshold, bit clock); what a
// bank does with the channel bits -- its tracker kernel, its state and records -- stays with the bank.
//
// Device: FrontArgs<Par> (what k_fsk_front reads and writes of a call), k_fsk_front, pll_step; the quantiser is
// kq::load_q (kq_tonecorr.hpp), whose 32-bit sample index holds every sample of a call: front_config keeps max_samples
// within 2^28.
//   k_fsk_front  one workgroup per (slot, tile of kTile samples on the grid of 64-sample words): tile and halo quantised into
//                LDS, the FIR, running max / min over W by doubling (log2 W steps whatever W is), the compare packed with
//                __ballot: one wave, one word.  The first tile of a slot also writes the q the next call starts from
// Host: design_taps, front_config (the checks of the fields the banks' configs share, and the geometry), FrontDev (taps,
// the two copies of the carried q, the packed decisions, the level), bind_front and launch_front.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_host.hpp"
#include "kq_slots.hpp"
#include "kq_tonecorr.hpp"

namespace kq {
namespace fskfront {

constexpr unsigned kMaxSlots = 4096;
constexpr int kMaxK = 127, kMaxW = 1024;
constexpr int kTile = 1024;                     // samples per workgroup of k_fsk_front: 16 words
constexpr int kThreads = 256;
constexpr int kMaxH = kMaxK - 1 + kMaxW - 1;    // halo
constexpr int kMaxY = kTile + kMaxW - 1;        // values of y a tile needs
constexpr int kPer = (kMaxY + kThreads - 1) / kThreads;

struct Geom {
  int K, W, H, HN;               // H = K - 1 + W - 1, HN = H + 63
  int P, off;                    // 2^P <= W < 2^(P + 1), off = W - 2^P
  unsigned inc;
  int pll_shift;
  float scale;
  int S;                         // max_slots
  size_t words;                  // per slot: max_samples / 64 + 2
};

// Par: the bank's per-slot record (kq::SlotTable), with `unsigned source`
template <class Par>
struct FrontArgs {
  Geom g;
  const Par *par;
  const int *list;               // active slots, ascending
  const short *taps;             // [K]
  const short *hist_in;          // [S][HN]: q[n0 - HN .. n0 - 1]
  short *hist_out;               // [S][HN]: q[n1 - HN .. n1 - 1]
  unsigned long long *dw;        // [words][S]: word w0 + i of slot s at i S + s
  unsigned *level;               // [S]
  int64_t n0, n1;                // the call's samples
  int64_t w0;                    // n0 / 64
  PcmIn in;
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
};

template <class Par>
__global__ __launch_bounds__(kThreads) void k_fsk_front(FrontArgs<Par> a) {
  __shared__ short q[kTile + kMaxH];
  __shared__ int mx[kMaxY], mn[kMaxY];
  __shared__ int ys[kTile];
  __shared__ int hs[kMaxK + 1];
  Geom const &g = a.g;
  int const li = blockIdx.y, slot = a.list[li], tid = threadIdx.x;
  size_t const row = a.rowmap ? (size_t)a.rowmap[li] : (size_t)a.par[slot].source;
  const short *hin = a.hist_in + (size_t)slot * g.HN;
  int64_t const t0 = 64 * a.w0 + (int64_t)blockIdx.x * kTile;     // the tile's first sample
  int64_t const wend = 64 * (((a.n1 - 1) >> 6) + 1);              // the end of the call's last word
  int const nT = (int)(wend - t0 < kTile ? wend - t0 : kTile);    // whole words
  int const nq = nT + g.H, ny = nT + g.W - 1;
  // q[i] = q of sample t0 - H + i: before the call from the carried ones, beyond it (the rest of the last word) zero
  for (int i = tid; i < nq; i += kThreads) {
    int64_t const n = t0 - g.H + i;
    int v = 0;
    if (n < a.n0) v = hin[g.HN - (int)(a.n0 - n)];
    else if (n < a.n1) v = load_q(a.in, row, (unsigned)(n - a.n0));  // (below max_samples <= 2^28)
    q[i] = (short)v;
  }
  for (int k = tid; k < g.K; k += kThreads) hs[k] = a.taps[k];
  if (blockIdx.x == 0) {  // the next call's carried q (the other copy: the tiles of this call still read this one)
    short *hout = a.hist_out + (size_t)slot * g.HN;
    int64_t const ncall = a.n1 - a.n0;
    for (int i = tid; i < g.HN; i += kThreads) {
      int64_t const n = a.n1 - g.HN + i;
      hout[i] = n < a.n0 ? hin[i + ncall] : (short)load_q(a.in, row, (unsigned)(n - a.n0));
    }
  }
  __syncthreads();
  // y of sample t0 - (W - 1) + i
  for (int i = tid; i < ny; i += kThreads) {
    int acc = 0;
    const short *qi = q + i + g.K - 1;
    for (int k = 0; k < g.K; k++) acc += hs[k] * (int)qi[-k];
    mx[i] = mn[i] = acc;
    if (i >= g.W - 1) ys[i - (g.W - 1)] = acc;
  }
  __syncthreads();
  // after step j, mx[i] = max y over the 2^(j + 1) samples ending at i (where that many exist; the others are not read)
  for (int j = 0; j < g.P; j++) {
    int const step = 1 << j;
    int hi[kPer], lo[kPer];
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const i = tid + t * kThreads;
      if (i < ny) {
        int const b = i >= step ? i - step : i;
        hi[t] = max(mx[i], mx[b]);
        lo[t] = min(mn[i], mn[b]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const i = tid + t * kThreads;
      if (i < ny) {
        mx[i] = hi[t];
        mn[i] = lo[t];
      }
    }
    __syncthreads();
  }
  // one wave, one word
  int const lane = tid & 63, nwords = nT >> 6;
  for (int w = tid >> 6; w < nwords; w += kThreads / 64) {
    int const j = 64 * w + lane, i = j + g.W - 1;
    int64_t const n = t0 + j;
    long long const top = max(mx[i], mx[i - g.off]), bot = min(mn[i], mn[i - g.off]);
    bool const d = n < a.n1 && 2 * (long long)ys[j] > top + bot;
    unsigned long long const word = __ballot(d);
    if (lane == 0) a.dw[(size_t)((t0 >> 6) + w - a.w0) * g.S + slot] = word;
    if (n == a.n1 - 1) a.level[slot] = (unsigned)(top - bot);
  }
}

// the bit clock at one sample: s and dprev move on; true when a channel bit (c = d) is taken at this sample
__device__ __forceinline__ bool pll_step(int &s, int &dprev, int d, Geom const &g) {
  if (d != dprev) s -= s >> g.pll_shift;
  dprev = d;
  long long const t = (long long)s + (long long)g.inc;
  if (t < 0x80000000LL) {
    s = (int)t;
    return false;
  }
  s = (int)(t - 0x100000000LL);
  return true;
}

// ---- host -----------------------------------------------------------------------------------------------------------
// hq: the Kaiser-windowed sinc in double, sum 1, times 32768 and rounded
inline std::vector<short> design_taps(int K, double cutoff, double Fs, double beta, long *sum_abs) {
  std::vector<double> h((size_t)K);
  double const den = kq::i0_double(M_PI * beta), c = 0.5 * (K - 1);
  double sum = 0;
  for (int k = 0; k < K; k++) {
    double const pp = 2.0 * k / (K - 1) - 1.0;  // make_kaiser, filter.c:337-357
    double const w = kq::i0_double(M_PI * beta * std::sqrt(std::max(0.0, 1.0 - pp * pp))) / den;
    double const t = 2.0 * cutoff / Fs * (k - c);
    h[k] = (t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t)) * w;
    sum += h[k];
  }
  std::vector<short> hq((size_t)K);
  *sum_abs = 0;
  for (int k = 0; k < K; k++) {
    long const v = std::lrint(h[k] / sum * 32768.0);
    *sum_abs += std::labs(v);
    hq[k] = (short)std::max(-32768L, std::min(32767L, v));
  }
  return hq;
}

// the fields that kq_fsk_config and kq_pag_config share, as kq_*_create checks them
struct FrontConfig {
  double samprate;
  int baud;
  unsigned taps;
  float cutoff_hz, kaiser_beta, window_bits, input_scale;
  int pll_shift;
  unsigned max_slots;
  size_t max_samples;
};

// The limits of the front end, in the order the header lists them; the reason goes to kq_last_error under fn's name.
// True: *g and *hq are the geometry and the quantised low-pass.  Touches no device.
inline bool front_config(const char *fn, FrontConfig const &c, Geom *g, std::vector<short> *hq) {
  if (c.baud <= 0 || !(c.samprate > 0) || !std::isfinite(c.samprate)) {
    kq_internal_set_error("%s: samprate %.10g and baud %d must be positive", fn, c.samprate, c.baud);
    return false;
  }
  double const Fs = c.samprate, baud = c.baud;
  if (Fs < 4 * baud || Fs > 40 * baud) {
    kq_internal_set_error("%s: samprate %.10g must be 4 .. 40 times baud %d", fn, c.samprate, c.baud);
    return false;
  }
  unsigned const K = c.taps;
  if (K < 3 || K > (unsigned)kMaxK || !(K & 1)) {
    kq_internal_set_error("%s: taps %u must be odd and 3..%d", fn, K, kMaxK);
    return false;
  }
  if (!std::isfinite(c.window_bits) || c.window_bits <= 0) {
    kq_internal_set_error("%s: window_bits must be finite and positive", fn);
    return false;
  }
  double const Wd = std::rint((double)c.window_bits * Fs / baud);
  if (Wd < 2 || Wd > kMaxW) {
    kq_internal_set_error("%s: window_bits %g gives W = %.0f samples, must be 2..%d", fn, (double)c.window_bits, Wd, kMaxW);
    return false;
  }
  if (!(c.cutoff_hz > 0) || !(c.cutoff_hz < 0.5 * Fs)) {
    kq_internal_set_error("%s: cutoff_hz %g must be above 0 and below samprate / 2", fn, (double)c.cutoff_hz);
    return false;
  }
  if (!std::isfinite(c.kaiser_beta) || c.kaiser_beta < 0) {
    kq_internal_set_error("%s: kaiser_beta must be finite and >= 0", fn);
    return false;
  }
  if (c.pll_shift < 1 || c.pll_shift > 8) {
    kq_internal_set_error("%s: pll_shift %d must be 1..8", fn, c.pll_shift);
    return false;
  }
  if (!input_scale_ok(fn, c.input_scale) || !field_in_range(fn, "max_slots", c.max_slots, 1, kMaxSlots) ||
      !max_samples_ok(fn, c.max_samples))
    return false;
  long sum_abs = 0;
  *hq = design_taps((int)K, c.cutoff_hz, Fs, c.kaiser_beta, &sum_abs);
  if (sum_abs > 65535) {
    kq_internal_set_error("%s: taps %u, cutoff_hz %g, kaiser_beta %g give sum |hq| = %ld > 65535: the filter could overflow", fn,
                          K, (double)c.cutoff_hz, (double)c.kaiser_beta, sum_abs);
    return false;
  }
  g->K = (int)K;
  g->W = (int)Wd;
  g->H = g->K - 1 + g->W - 1;
  g->HN = g->H + 63;
  g->P = 0;
  while ((2 << g->P) <= g->W) g->P++;
  g->off = g->W - (1 << g->P);
  g->inc = (unsigned)std::llrint(4294967296.0 * baud / Fs);
  g->pll_shift = c.pll_shift;
  g->scale = c.input_scale;
  g->S = (int)c.max_slots;
  g->words = c.max_samples / 64 + 2;
  return true;
}

// what the front end keeps on the device (part of a bank's kq::lazy_device half)
struct FrontDev {
  short *taps = nullptr;
  short *hist[2] = {nullptr, nullptr};
  unsigned long long *dw = nullptr;
  unsigned *level = nullptr;

  // (the caller waits for the stream before the taps' host copy may go)
  int alloc(HostSide &h, Geom const &g, std::vector<short> const &hq) {
    size_t const S = (size_t)g.S;
    if (h.alloc(&taps, (size_t)g.K) || h.alloc(&hist[0], S * g.HN, true) || h.alloc(&hist[1], S * g.HN, true) ||
        h.alloc(&dw, g.words * S) || h.alloc(&level, S, true))
      return -1;
    KQ_TRY(hipMemcpyAsync(taps, hq.data(), hq.size() * sizeof(short), hipMemcpyHostToDevice, h.stream));
    return 0;
  }

  // zero history and level of one slot
  int cold_start(HostSide &h, Geom const &g, unsigned s) {
    for (short *p : hist) KQ_TRY(hipMemsetAsync(p + (size_t)s * g.HN, 0, g.HN * sizeof(short), h.stream));
    KQ_TRY(hipMemsetAsync(level + s, 0, sizeof(unsigned), h.stream));
    return 0;
  }
};

// A call's FrontArgs: `turn` is the copy of the carried q the call reads; the input as kq::bind_pcm binds it
template <class Par>
int bind_front(FrontArgs<Par> *a, HostSide &h, SlotTable<Par> &slots, FrontDev const &d, Geom const &g, int turn, uint64_t n_cur,
               size_t max_samples, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
               unsigned nblocks, int on_device) {
  a->g = g;
  a->par = slots.d_par;
  a->list = slots.d_list;
  a->taps = d.taps;
  a->hist_in = d.hist[turn];
  a->hist_out = d.hist[turn ^ 1];
  a->dw = d.dw;
  a->level = d.level;
  a->n0 = (int64_t)n_cur;
  a->n1 = a->n0 + (int64_t)block_len * nblocks;
  a->w0 = a->n0 >> 6;
  return bind_pcm(&a->in, &a->rowmap, h, slots, max_samples, g.scale, src, format, src_stride, row_stride, block_len, nblocks, on_device);
}

template <class Par>
int launch_front(FrontArgs<Par> const &a, size_t nlist, hipStream_t stream) {
  int64_t const nwords = ((a.n1 - 1) >> 6) - a.w0 + 1;  // <= max_samples / 64 + 2
  unsigned const tiles = (unsigned)((nwords * 64 + kTile - 1) / kTile);
  hipLaunchKernelGGL(k_fsk_front<Par>, dim3(tiles, (unsigned)nlist), dim3(kThreads), 0, stream, a);
  KQ_TRY(hipGetLastError());
  return 0;
}

}  // namespace fskfront
}  // namespace kq
