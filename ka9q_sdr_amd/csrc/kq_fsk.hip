// kq_fsk.hip -- baseband FSK / GMSK packet decoder bank: flat FM discriminator output -> HDLC frames (9600 bit/s G3RUH,
// AIS) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_fsk_*): q = the input quantised to int16, y = hq * q in int32, d[n] = (2 y[n] > max + min
// of y over the last W samples), a shift DPLL that takes a channel bit per symbol, descrambler, NRZI, HDLC deframer with
// the CRC-16/X.25 check.  All integer after the quantiser, so nothing depends on the order of a sum.  State on the device,
// per slot: the last HN = K - 1 + W - 1 + 63 values of q (two copies, written in turn: a call reads one and writes the other),
// the call's d packed 64 samples to a word, FskState, the open frame, the arena of good frames.
//
// k_fsk_front  one workgroup per (slot, tile of kTile samples on the grid of 64-sample words): tile and halo quantised into
//              LDS, the FIR, running max / min over W by doubling (log2 W steps whatever W is), the compare packed with
//              __ballot: one wave, one word.  The first tile of a slot also writes the q the next call starts from
// k_fsk_track  one lane per slot: the call's words in order through DPLL, descrambler, NRZI and deframer; frames and status
//              out.  Serial by nature, as k_rds_track is; the open frame lives in global memory, written a byte at a time
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_slots.hpp"

namespace {

constexpr unsigned kMaxSlots = 4096;
constexpr int kMaxK = 127, kMaxW = 1024;
constexpr int kTile = 1024;                     // samples per workgroup of k_fsk_front: 16 words
constexpr int kThreads = 256;
constexpr int kMaxH = kMaxK - 1 + kMaxW - 1;    // halo
constexpr int kMaxY = kTile + kMaxW - 1;        // values of y a tile needs
constexpr int kPer = (kMaxY + kThreads - 1) / kThreads;

struct FskPar {  // per slot, written by the host at kq_fsk_set
  int active;
  unsigned source;
  int scrambled;
  int min_bytes;
};

struct FskState {  // per slot, carried from call to call; all zero when a slot is set
  int s;                         // the bit clock
  unsigned sr;                   // descrambler
  int dprev, uprev;
  int ones, in_frame, nbits;
  unsigned cur;                  // the open byte
  unsigned crc_run, crc_byte;    // CRC register over the bits appended so far / at the last byte boundary
  unsigned bits, frames_good, frames_bad, aborts, dropped;
  int pad;
};

struct FskGeom {
  int K, W, H, HN;               // H = K - 1 + W - 1, HN = H + 63
  int P, off;                    // 2^P <= W < 2^(P + 1), off = W - 2^P
  unsigned inc;
  int pll_shift;
  float scale;
  int max_frames, mfb;
  int S;                         // max_slots
  size_t words;                  // per slot: max_samples / 64 + 2
};

struct CallArgs {
  FskGeom g;
  const FskPar *par;
  const int *list;               // active slots, ascending
  const short *taps;             // [K]
  const short *hist_in;          // [S][HN]: q[n0 - HN .. n0 - 1]
  short *hist_out;               // [S][HN]: q[n1 - HN .. n1 - 1]
  unsigned long long *dw;        // [words][S]: word w0 + i of slot s at i S + s
  unsigned *level;               // [S]
  FskState *state;               // [S]
  unsigned char *open;           // [S][mfb]
  unsigned char *frames;         // [S][max_frames][mfb]
  kq_fsk_frame_info *info;       // [S][max_frames]
  unsigned *nframes;             // [S]
  int64_t n0, n1;                // the call's samples
  int64_t w0;                    // n0 / 64
  // input
  const void *src;
  int format;
  size_t src_stride, row_stride;
  unsigned block_len;
  const int *rowmap;             // per list entry: the row of `src` (host input, staged) or null (par.source)
  // output
  kq_fsk_status *st;
  size_t sstride;
};

// q of the call's i-th sample
__device__ __forceinline__ int load_q(CallArgs const &a, size_t row, size_t i) {
  size_t const k = i / a.block_len, j = i - k * a.block_len;
  size_t const idx = row * a.src_stride + k * a.row_stride + j;
  if (a.format == KQ_PCM_S16BE) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a.src) + 2 * idx;
    int const w = (int)(short)(unsigned short)(((unsigned)p[0] << 8) | p[1]);
    return w < -32767 ? -32767 : w;
  }
  float const v = rintf(reinterpret_cast<const float *>(a.src)[idx] * a.g.scale);
  if (!(v == v)) return 0;
  return (int)fminf(fmaxf(v, -32767.f), 32767.f);
}

__global__ __launch_bounds__(kThreads) void k_fsk_front(CallArgs a) {
  __shared__ short q[kTile + kMaxH];
  __shared__ int mx[kMaxY], mn[kMaxY];
  __shared__ int ys[kTile];
  __shared__ int hs[kMaxK + 1];
  FskGeom const &g = a.g;
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
    else if (n < a.n1) v = load_q(a, row, (size_t)(n - a.n0));
    q[i] = (short)v;
  }
  for (int k = tid; k < g.K; k += kThreads) hs[k] = a.taps[k];
  if (blockIdx.x == 0) {  // the next call's carried q (the other copy: the tiles of this call still read this one)
    short *hout = a.hist_out + (size_t)slot * g.HN;
    int64_t const ncall = a.n1 - a.n0;
    for (int i = tid; i < g.HN; i += kThreads) {
      int64_t const n = a.n1 - g.HN + i;
      hout[i] = n < a.n0 ? hin[i + ncall] : (short)load_q(a, row, (size_t)(n - a.n0));
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

struct FrameOut {
  unsigned char *open;
  unsigned char *frames;
  kq_fsk_frame_info *info;
  unsigned n;                    // frames in the arena
};

__device__ __forceinline__ void append(FskState &s, unsigned bit, int mfb, unsigned char *open) {
  if (s.nbits < 8 * mfb) {
    s.cur |= bit << (s.nbits & 7);
    s.crc_run = (s.crc_run >> 1) ^ (((s.crc_run ^ bit) & 1u) ? 0x8408u : 0u);
    if ((s.nbits & 7) == 7) {
      open[s.nbits >> 3] = (unsigned char)s.cur;
      s.cur = 0;
      s.crc_byte = s.crc_run;
    }
  }
  if (s.nbits < 0x7FFFFFFF) s.nbits++;
}

// one data bit through the deframer (the header's "HDLC")
__device__ __forceinline__ void push_bit(FskState &s, unsigned b, FskPar const &p, FskGeom const &g, FrameOut &o, int64_t n) {
  if (b) {
    if (s.ones < 7) s.ones++;
    if (s.ones == 7) {
      if (s.in_frame) s.aborts++;
      s.in_frame = 0;
    } else if (s.in_frame) {
      append(s, 1u, g.mfb, o.open);
    }
    return;
  }
  if (s.ones == 6) {
    int const nb = s.nbits - 7;
    if (s.in_frame && nb >= 8 * p.min_bytes) {
      int const len = nb >> 3;
      if ((nb & 7) == 0 && len <= g.mfb && s.crc_byte == 0xf0b8u) {
        s.frames_good++;
        if (o.n < (unsigned)g.max_frames) {
          unsigned char *dst = o.frames + (size_t)o.n * g.mfb;
          for (int i = 0; i < len; i++) dst[i] = o.open[i];
          kq_fsk_frame_info r;
          r.length = (uint32_t)len;
          r.end_bit = s.bits;
          r.end_sample = (uint64_t)n;
          o.info[o.n] = r;
          o.n++;
        } else {
          s.dropped++;
        }
      } else {
        s.frames_bad++;
      }
    }
    s.in_frame = 1;
    s.nbits = 0;
    s.cur = 0;
    s.crc_run = s.crc_byte = 0xFFFFu;
  } else if (s.ones < 5 && s.in_frame) {
    append(s, 0u, g.mfb, o.open);
  }
  s.ones = 0;
}

// one lane per slot: the call's samples in order
__global__ __launch_bounds__(64) void k_fsk_track(CallArgs a, int nlist) {
  int const li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nlist) return;
  int const slot = a.list[li];
  FskGeom const &g = a.g;
  FskPar const p = a.par[slot];
  FskState s = a.state[slot];
  FrameOut o;
  o.open = a.open + (size_t)slot * g.mfb;
  o.frames = a.frames + (size_t)slot * g.max_frames * g.mfb;
  o.info = a.info + (size_t)slot * g.max_frames;
  o.n = a.nframes[slot];
  int64_t n = a.n0;
  while (n < a.n1) {
    int const b0 = (int)(n & 63);
    int64_t const left = a.n1 - n;
    int const cnt = (int)(left < 64 - b0 ? left : 64 - b0);
    unsigned long long word = a.dw[(size_t)((n >> 6) - a.w0) * g.S + slot] >> b0;
    for (int k = 0; k < cnt; k++, word >>= 1, n++) {
      int const d = (int)(word & 1u);
      if (d != s.dprev) s.s -= s.s >> g.pll_shift;
      s.dprev = d;
      long long const t = (long long)s.s + (long long)g.inc;
      if (t < 0x80000000LL) {
        s.s = (int)t;
        continue;
      }
      s.s = (int)(t - 0x100000000LL);
      s.bits++;
      unsigned const c = (unsigned)d;
      unsigned u = c;
      if (p.scrambled) {
        u = c ^ ((s.sr >> 16) & 1u) ^ ((s.sr >> 11) & 1u);
        s.sr = ((s.sr << 1) | c) & 0x1FFFFu;
      }
      unsigned const b = u == (unsigned)s.uprev;
      s.uprev = (int)u;
      push_bit(s, b, p, g, o, n);
    }
  }
  a.state[slot] = s;
  a.nframes[slot] = o.n;
  if (a.st) {
    kq_fsk_status r;
    r.bits = s.bits;
    r.frames_good = s.frames_good;
    r.frames_bad = s.frames_bad;
    r.aborts = s.aborts;
    r.dropped = s.dropped;
    r.pll_phase = s.s;
    r.in_frame = s.in_frame;
    r.level = a.level[slot];
    a.st[(size_t)slot * a.sstride] = r;
  }
}

// hq: the Kaiser-windowed sinc in double, sum 1, times 32768 and rounded
std::vector<short> design_taps(int K, double cutoff, double Fs, double beta, long *sum_abs) {
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

}  // namespace

struct kq_fsk_bank : kq::HostSide {
  kq_fsk_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  FskGeom g{};
  uint64_t n_cur = 0;
  int turn = 0;                          // the copy of the carried q the next call reads
  std::vector<short> hq;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<FskPar> slots;
    short *taps = nullptr;
    short *hist[2] = {nullptr, nullptr};
    unsigned long long *dw = nullptr;
    unsigned *level = nullptr;
    FskState *state = nullptr;
    unsigned char *open = nullptr, *frames = nullptr;
    kq_fsk_frame_info *info = nullptr;
    unsigned *nframes = nullptr;
    kq_fsk_status *st = nullptr;         // host-memory calls
  } d;
};

namespace {

int make_device(kq_fsk_bank *b) {
  kq_fsk_config const &c = b->cfg;
  FskGeom const &g = b->g;
  auto &d = b->d;
  if (b->open_stream(c.stream)) return -1;
  size_t const S = c.max_slots;
  if (d.slots.alloc(*b, S) || b->alloc(&d.taps, (size_t)g.K) || b->alloc(&d.hist[0], S * g.HN, true) ||
      b->alloc(&d.hist[1], S * g.HN, true) || b->alloc(&d.dw, g.words * S) || b->alloc(&d.level, S, true) ||
      b->alloc(&d.state, S, true) || b->alloc(&d.open, S * g.mfb, true) || b->alloc(&d.frames, S * g.max_frames * g.mfb) ||
      b->alloc(&d.info, S * g.max_frames) || b->alloc(&d.nframes, S, true))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.taps, b->hq.data(), b->hq.size() * sizeof(short), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// zero history, clock, deframer and arena (the stream is idle: callers synchronised it)
int cold_start(kq_fsk_bank *b, unsigned s) {
  for (short *h : b->d.hist) KQ_TRY(hipMemsetAsync(h + (size_t)s * b->g.HN, 0, b->g.HN * sizeof(short), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.state + s, 0, sizeof(FskState), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.nframes + s, 0, sizeof(unsigned), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.level + s, 0, sizeof(unsigned), b->stream));
  return 0;
}

}  // namespace

extern "C" {

kq_fsk_bank *kq_fsk_create(const kq_fsk_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_fsk_create: null config");
    return nullptr;
  }
  if (cfg->baud <= 0 || cfg->samprate <= 0) {
    kq_internal_set_error("kq_fsk_create: samprate %d and baud %d must be positive", cfg->samprate, cfg->baud);
    return nullptr;
  }
  long long const Fs = cfg->samprate, baud = cfg->baud;
  if (Fs < 4 * baud || Fs > 40 * baud) {
    kq_internal_set_error("kq_fsk_create: samprate %d must be 4 .. 40 times baud %d", cfg->samprate, cfg->baud);
    return nullptr;
  }
  unsigned const K = cfg->taps;
  if (K < 3 || K > (unsigned)kMaxK || !(K & 1)) {
    kq_internal_set_error("kq_fsk_create: taps %u must be odd and 3..%d", K, kMaxK);
    return nullptr;
  }
  if (!std::isfinite(cfg->window_bits) || cfg->window_bits <= 0) {
    kq_internal_set_error("kq_fsk_create: window_bits must be finite and positive");
    return nullptr;
  }
  double const Wd = std::rint((double)cfg->window_bits * (double)Fs / (double)baud);
  if (Wd < 2 || Wd > kMaxW) {
    kq_internal_set_error("kq_fsk_create: window_bits %g gives W = %.0f samples, must be 2..%d", (double)cfg->window_bits, Wd, kMaxW);
    return nullptr;
  }
  if (!(cfg->cutoff_hz > 0) || !(cfg->cutoff_hz < 0.5 * (double)Fs)) {
    kq_internal_set_error("kq_fsk_create: cutoff_hz %g must be above 0 and below samprate / 2", (double)cfg->cutoff_hz);
    return nullptr;
  }
  if (!std::isfinite(cfg->kaiser_beta) || cfg->kaiser_beta < 0) {
    kq_internal_set_error("kq_fsk_create: kaiser_beta must be finite and >= 0");
    return nullptr;
  }
  if (cfg->pll_shift < 1 || cfg->pll_shift > 8) {
    kq_internal_set_error("kq_fsk_create: pll_shift %d must be 1..8", cfg->pll_shift);
    return nullptr;
  }
  if (!std::isfinite(cfg->input_scale) || !(cfg->input_scale > 0)) {
    kq_internal_set_error("kq_fsk_create: input_scale must be finite and positive");
    return nullptr;
  }
  if (cfg->max_slots == 0 || cfg->max_slots > kMaxSlots) {
    kq_internal_set_error("kq_fsk_create: max_slots %u must be 1..%u", cfg->max_slots, kMaxSlots);
    return nullptr;
  }
  if (cfg->max_frames == 0 || cfg->max_frames > 4096) {
    kq_internal_set_error("kq_fsk_create: max_frames %u must be 1..4096", cfg->max_frames);
    return nullptr;
  }
  if (cfg->max_frame_bytes < 8 || cfg->max_frame_bytes > 1024) {
    kq_internal_set_error("kq_fsk_create: max_frame_bytes %u must be 8..1024", cfg->max_frame_bytes);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_fsk_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  long sum_abs = 0;
  std::vector<short> hq = design_taps((int)K, cfg->cutoff_hz, (double)Fs, cfg->kaiser_beta, &sum_abs);
  if (sum_abs > 65535) {
    kq_internal_set_error("kq_fsk_create: taps %u, cutoff_hz %g, kaiser_beta %g give sum |hq| = %ld > 65535: the filter could overflow",
                          K, (double)cfg->cutoff_hz, (double)cfg->kaiser_beta, sum_abs);
    return nullptr;
  }
  kq_fsk_bank *b = new kq_fsk_bank;
  b->cfg = *cfg;
  b->hq = std::move(hq);
  FskGeom &g = b->g;
  g.K = (int)K;
  g.W = (int)Wd;
  g.H = g.K - 1 + g.W - 1;
  g.HN = g.H + 63;
  g.P = 0;
  while ((2 << g.P) <= g.W) g.P++;
  g.off = g.W - (1 << g.P);
  g.inc = (unsigned)std::llrint(4294967296.0 * (double)baud / (double)Fs);
  g.pll_shift = cfg->pll_shift;
  g.scale = cfg->input_scale;
  g.max_frames = (int)cfg->max_frames;
  g.mfb = (int)cfg->max_frame_bytes;
  g.S = (int)cfg->max_slots;
  g.words = cfg->max_samples / 64 + 2;
  return b;
}

int kq_fsk_destroy(kq_fsk_bank *b) { return kq::destroy_bank(b, "kq_fsk_destroy"); }

int kq_fsk_set(kq_fsk_bank *b, unsigned slot, const kq_fsk_params *p) {
  if (!kq::set_args_ok("kq_fsk_set", slot, p, kMaxSlots)) return -1;
  if (p->min_bytes < 4) {
    kq_internal_set_error("kq_fsk_set: min_bytes %u must be >= 4", p->min_bytes);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_fsk_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (p->min_bytes > b->cfg.max_frame_bytes) {
    kq_internal_set_error("kq_fsk_set: min_bytes %u > max_frame_bytes %u", p->min_bytes, b->cfg.max_frame_bytes);
    return -1;
  }
  if (!kq::slot_in_bank("kq_fsk_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  FskPar np{};
  np.active = 1;
  np.source = p->source;
  np.scrambled = p->scrambled != 0;
  np.min_bytes = (int)p->min_bytes;
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_fsk_remove(kq_fsk_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_fsk_remove"); }

int kq_fsk_process(kq_fsk_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_fsk_status *status, size_t status_stride) {
  if (!b) {
    kq_internal_set_error("kq_fsk_process: null bank");
    return -1;
  }
  if (format != KQ_PCM_F32 && format != KQ_PCM_S16BE) {
    kq_internal_set_error("kq_fsk_process: unknown sample format %d", format);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_fsk_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  if (status && status_stride < 1) {
    kq_internal_set_error("kq_fsk_process: status_stride %zu < 1", status_stride);
    return -1;
  }
  kq::CallWork const work = kq::call_work(b, "kq_fsk_process", ncall, src, "src");
  if (work == kq::CALL_IDLE) {
    b->n_cur += ncall;
    return 0;
  }
  if (work != kq::CALL_RUN) return work;
  kq::DeviceScope dev_scope_(b->cfg.device);
  FskGeom const &g = b->g;
  auto &d = b->d;
  size_t const S = b->cfg.max_slots, nlist = d.slots.all.size();
  CallArgs a{};
  a.g = g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.taps = d.taps;
  a.hist_in = d.hist[b->turn];
  a.hist_out = d.hist[b->turn ^ 1];
  a.dw = d.dw;
  a.level = d.level;
  a.state = d.state;
  a.open = d.open;
  a.frames = d.frames;
  a.info = d.info;
  a.nframes = d.nframes;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  a.w0 = a.n0 >> 6;
  a.format = format;
  a.block_len = block_len;
  if (on_device) {
    a.src = src;
    a.src_stride = src_stride;
    a.row_stride = row_stride;
    a.rowmap = nullptr;
    a.st = status;
    a.sstride = status_stride;
  } else {
    // (the stage holds 4 bytes per sample whatever the format; the rows lie as closely as the format allows)
    kq::Staged in;
    if (d.slots.stage_rows(*b, src, format == KQ_PCM_S16BE ? 2 : 4, src_stride, row_stride, block_len, nblocks,
                           b->cfg.max_samples * 4, &in))
      return -1;
    a.src = in.src;
    a.src_stride = in.src_stride;
    a.row_stride = in.row_stride;
    a.rowmap = in.rowmap;
    if (status && !d.st && b->alloc(&d.st, S)) return -1;
    a.st = status ? d.st : nullptr;
    a.sstride = 1;
  }
  int64_t const nwords = ((a.n1 - 1) >> 6) - a.w0 + 1;  // <= max_samples / 64 + 2
  unsigned const tiles = (unsigned)((nwords * 64 + kTile - 1) / kTile);
  hipLaunchKernelGGL(k_fsk_front, dim3(tiles, (unsigned)nlist), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fsk_track, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, b->stream, a, (int)nlist);
  KQ_TRY(hipGetLastError());
  b->turn ^= 1;  // from here on the carried q is in the other copy, whatever fails below
  b->n_cur += ncall;
  if (!on_device) {
    auto back = [&](size_t s0, size_t n) {  // the records of the active slots
      return kq::copy_rows_back(*b, status, status_stride, d.st, 1, 1, sizeof(kq_fsk_status), s0, n);
    };
    if (status && d.slots.for_runs(back)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  return 0;
}

int kq_fsk_pull_counts(kq_fsk_bank *b, uint32_t *counts) {
  if (!b) {
    kq_internal_set_error("kq_fsk_pull_counts: null bank");
    return -1;
  }
  if (!counts) {
    kq_internal_set_error("kq_fsk_pull_counts: null counts");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) {
    std::memset(counts, 0, b->cfg.max_slots * sizeof(uint32_t));
    return 0;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipMemcpyAsync(counts, b->d.nframes, b->cfg.max_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_fsk_pull_frame(kq_fsk_bank *b, unsigned slot, unsigned index, unsigned char *dst, size_t cap, kq_fsk_frame_info *info) {
  if (!b) {
    kq_internal_set_error("kq_fsk_pull_frame: null bank");
    return -1;
  }
  if (!dst) {
    kq_internal_set_error("kq_fsk_pull_frame: null dst");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots) {
    kq_internal_set_error("kq_fsk_pull_frame: slot %u >= max_slots %u", slot, b->cfg.max_slots);
    return -1;
  }
  unsigned n = 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (b->dev_ready) {
    KQ_TRY(hipMemcpyAsync(&n, b->d.nframes + slot, sizeof n, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (index >= n) {
    kq_internal_set_error("kq_fsk_pull_frame: slot %u has %u frames", slot, n);
    return -1;
  }
  size_t const at = (size_t)slot * b->g.max_frames + index;
  kq_fsk_frame_info r;
  KQ_TRY(hipMemcpyAsync(&r, b->d.info + at, sizeof r, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  size_t const take = std::min(cap, (size_t)r.length);
  if (take) {
    KQ_TRY(hipMemcpyAsync(dst, b->d.frames + at * b->g.mfb, take, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (info) *info = r;
  return (int)r.length;
}

int kq_fsk_clear_frames(kq_fsk_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_fsk_clear_frames: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipMemsetAsync(b->d.nframes, 0, b->cfg.max_slots * sizeof(unsigned), b->stream));
  return 0;
}

int kq_fsk_get_taps(const kq_fsk_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_fsk_get_taps: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_fsk_get_taps: null dst");
    return -1;
  }
  size_t const n = std::min(cap, b->hq.size());
  if (n) std::memcpy(dst, b->hq.data(), n * sizeof(int16_t));
  return (int)b->hq.size();
}

int kq_fsk_sync(kq_fsk_bank *b) { return kq::sync_bank(b, "kq_fsk_sync"); }

int kq_fsk_reset(kq_fsk_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_fsk_reset: null bank");
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
