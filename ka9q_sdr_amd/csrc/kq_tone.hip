// kq_tone.hip -- tone signalling decoder bank: the audio of voice channels -> DTMF keys, the tones of five-tone selective
// calls and two-tone pages, as events (symbol, blocks, start, peak) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_tone_*): quantise as kq_fsk_*, correlate every block of B samples against up to 32
// tones from a 1024-entry cosine table with phases that are a function of the sample index alone, decide a symbol per block
// from the powers, and gather runs of equal symbols into events.  All exact integers after the quantiser.  State on the
// device, per slot: the I, Q, E of the open block, the last completed block's powers, ToneState (run, counters), the arena
// of events; per bank the table and the phase increments.
//
// k_tone  one workgroup per slot.  The call's samples go through LDS once, a piece at a time (a piece ends with its block,
//         the call or the tile), quantised as they are loaded.  Lanes split tones x sample phases: lane (t, p) of Tpad x
//         256 / Tpad takes samples p, p + 256 / Tpad, ... of the piece against tone t, two 64-bit multiply-adds a sample.
//         Where a block or the call ends the partial sums are folded: across the lanes of a wave by shuffles, across the
//         four waves through LDS, onto the carried sums that lanes 0 .. T - 1 hold in registers.  At a completed block
//         those lanes square, and lane 0 decides and steps the run: T compares from LDS, once per B samples, too small for
//         a kernel of its own, which would need every block's powers in memory (max_samples / B + 2 of them per slot).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_slots.hpp"
#include "kq_tonecorr.hpp"

namespace {

constexpr unsigned kMaxSlots = 4096;
constexpr int kMaxTones = 32;
using kq::tonecorr::kTable;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 2048;                     // samples in LDS at a time

struct ToneGeom {
  int B, T, Tpad;                // Tpad: the power of two >= T
  int g0, g1;
  unsigned long long min_e;      // min_ms B
  unsigned frac, ratio, twist, min_blocks;
  int max_events;
};

struct TonePar {  // per slot, written by the host at kq_tone_set
  int active;
  unsigned source;
};

struct ToneState {  // per slot, carried from call to call
  int cur;
  unsigned run;
  unsigned long long start, peak, energy;
  unsigned blocks, valid, events, dropped;
};

struct CallArgs {
  ToneGeom g;
  const TonePar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;            // [1024]
  const unsigned *incs;          // [T]
  ToneState *state;              // [S]
  long long *acc;                // [S][2 T + 1]: I, Q, E of the open block
  unsigned long long *last;      // [S][T]: P of the last completed block
  kq_tone_event *ev;             // [S][max_events]
  unsigned *nev;                 // [S]
  int64_t n0, n1;                // the call's samples
  kq::PcmIn in;
  // output
  kq_tone_status *st;
  size_t sstride;
  unsigned long long *pw;
  size_t pstride;
};

// of P[lo .. hi - 1]: the lowest index that attains the maximum, its P, and the largest of the others (0 if none)
__device__ __forceinline__ void group_best(const unsigned long long *P, int lo, int hi, int *best, unsigned long long *pb,
                                           unsigned long long *p2) {
  int b = lo;
  for (int i = lo + 1; i < hi; i++)
    if (P[i] > P[b]) b = i;
  unsigned long long second = 0;
  for (int i = lo; i < hi; i++)
    if (i != b && P[i] > second) second = P[i];
  *best = b - lo;
  *pb = P[b];
  *p2 = second;
}

// the header's "decide": the symbol of a completed block, or -1
__device__ __forceinline__ int decide(ToneGeom const &g, const unsigned long long *P, unsigned long long E) {
  unsigned long long const floor_ = ((E * (unsigned long long)g.B) >> 8) * g.frac;
  int i0, i1 = 0;
  unsigned long long pb0, p20;
  group_best(P, 0, g.g0, &i0, &pb0, &p20);
  bool ok = E >= g.min_e && pb0 >= floor_ && pb0 >= (p20 >> 4) * g.ratio;
  if (g.g1) {
    unsigned long long pb1, p21;
    group_best(P, g.g0, g.g0 + g.g1, &i1, &pb1, &p21);
    unsigned long long const hi = pb0 > pb1 ? pb0 : pb1, lo = pb0 > pb1 ? pb1 : pb0;
    ok = ok && pb1 >= floor_ && pb1 >= (p21 >> 4) * g.ratio && hi <= (lo >> 4) * g.twist;
  }
  return ok ? (i0 | (i1 << 8)) : -1;
}

// the header's "runs": block k with symbol sym and energy E
__device__ __forceinline__ void step_run(ToneGeom const &g, ToneState &s, int sym, unsigned long long E, int64_t k,
                                         kq_tone_event *ev, unsigned &nev) {
  s.blocks++;
  if (sym >= 0) s.valid++;
  s.energy = E;
  if (sym == s.cur) {
    if (s.run != 0xFFFFFFFFu) s.run++;
    if (E > s.peak) s.peak = E;
    return;
  }
  if (s.cur >= 0 && s.run >= g.min_blocks) {
    s.events++;
    if (nev >= (unsigned)g.max_events) {
      s.dropped++;
    } else {
      kq_tone_event r;
      r.symbol = s.cur;
      r.blocks = s.run;
      r.start_sample = s.start * (unsigned long long)g.B;
      r.peak = s.peak;
      ev[nev++] = r;
    }
  }
  s.cur = sym;
  s.run = 1;
  s.start = (unsigned long long)k;
  s.peak = E;
}

__global__ __launch_bounds__(kThreads) void k_tone(CallArgs c) {
  __shared__ short C[kTable];
  __shared__ short q[kTile];
  __shared__ long long red[kWaves][2 * kMaxTones + 1];
  __shared__ unsigned long long Ps[kMaxTones];
  ToneGeom const &g = c.g;
  int const li = blockIdx.x, slot = c.list[li], tid = threadIdx.x, wave = tid >> 6;
  size_t const row = c.rowmap ? (size_t)c.rowmap[li] : (size_t)c.par[slot].source;
  int const T = g.T, t = tid & (g.Tpad - 1), p = tid / g.Tpad, NP = kThreads / g.Tpad;
  bool const live = t < T;
  for (int i = tid; i < kTable; i += kThreads) C[i] = c.table[i];
  unsigned const inc = live ? c.incs[t] : 0u, step = (unsigned)NP * inc;
  // carried: lanes 0 .. T - 1 the open block's I and Q and the last block's P, lane 0 its E and the run
  long long *acc = c.acc + (size_t)slot * (2 * T + 1);
  long long cI = 0, cQ = 0, cE = 0;
  unsigned long long lastP = 0;
  ToneState s{};
  unsigned nev = 0;
  kq_tone_event *ev = c.ev + (size_t)slot * g.max_events;
  if (tid < T) {
    cI = acc[tid];
    cQ = acc[T + tid];
    lastP = c.last[(size_t)slot * T + tid];
  }
  if (tid == 0) {
    cE = acc[2 * T];
    s = c.state[slot];
    nev = c.nev[slot];
  }
  long long sI = 0, sQ = 0, sE = 0;
  int64_t n = c.n0, k = c.n0 / g.B, bend = (k + 1) * g.B;
  while (n < c.n1) {  // one piece: to the end of its block, of the call or of the tile
    int64_t e = bend < c.n1 ? bend : c.n1;
    if (e > n + kTile) e = n + kTile;
    int const len = (int)(e - n);
    __syncthreads();  // the piece before is done with q (and the first finds C loaded)
    for (int i = tid; i < len; i += kThreads) q[i] = (short)kq::load_q(c.in, row, (unsigned)(n - c.n0) + (unsigned)i);
    __syncthreads();
    if (live) {
      unsigned ph = ((unsigned)n + (unsigned)p) * inc;  // (n inc) mod 2^32 needs n mod 2^32 only
      for (int i = p; i < len; i += NP, ph += step) {
        int const j = (int)(ph >> 22), v = q[i];
        sI += (long long)v * C[j];
        sQ += (long long)v * C[(j - 256) & (kTable - 1)];
        if (t == 0) sE += (long long)v * v;
      }
    }
    n = e;
    if (n != bend && n != c.n1) continue;
    // fold the partial sums onto the carried ones: the lanes of a wave that share t are Tpad apart
    for (int off = 32; off >= g.Tpad; off >>= 1) {
      sI += __shfl_xor(sI, off);
      sQ += __shfl_xor(sQ, off);
      sE += __shfl_xor(sE, off);
    }
    if ((tid & 63) < g.Tpad && live) {
      red[wave][t] = sI;
      red[wave][kMaxTones + t] = sQ;
      if (t == 0) red[wave][2 * kMaxTones] = sE;
    }
    sI = sQ = sE = 0;
    __syncthreads();
    if (tid < T) {
      for (int w = 0; w < kWaves; w++) {
        cI += red[w][tid];
        cQ += red[w][kMaxTones + tid];
      }
    }
    if (tid == 0)
      for (int w = 0; w < kWaves; w++) cE += red[w][2 * kMaxTones];
    if (n == bend) {
      if (tid < T) {
        long long const a = cI >> 15, b = cQ >> 15;
        lastP = (unsigned long long)(a * a) + (unsigned long long)(b * b);
        Ps[tid] = lastP;
        cI = cQ = 0;
      }
      __syncthreads();
      if (tid == 0) {
        step_run(g, s, decide(g, Ps, (unsigned long long)cE), (unsigned long long)cE, k, ev, nev);
        cE = 0;
      }
      k++;
      bend += g.B;
    }
  }
  if (tid < T) {
    acc[tid] = cI;
    acc[T + tid] = cQ;
    c.last[(size_t)slot * T + tid] = lastP;
    if (c.pw) c.pw[(size_t)slot * c.pstride + tid] = lastP;
  }
  if (tid == 0) {
    acc[2 * T] = cE;
    c.state[slot] = s;
    c.nev[slot] = nev;
    if (c.pw) c.pw[(size_t)slot * c.pstride + T] = s.energy;
    if (c.st) {
      kq_tone_status r;
      r.blocks = s.blocks;
      r.valid_blocks = s.valid;
      r.events = s.events;
      r.dropped = s.dropped;
      r.cur = s.cur;
      r.run = s.run;
      r.energy = s.energy;
      c.st[(size_t)slot * c.sstride] = r;
    }
  }
}

}  // namespace

struct kq_tone_bank : kq::HostSide {
  static constexpr bool kDeferred = false;
  kq_tone_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  ToneGeom g{};
  std::vector<float> freqs;
  std::vector<unsigned> incs;
  uint64_t n_cur = 0;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<TonePar> slots;
    short *table = nullptr;
    unsigned *incs = nullptr;
    ToneState *state = nullptr;
    long long *acc = nullptr;
    unsigned long long *last = nullptr;
    kq::EventArena<kq_tone_event> arena;
    kq_tone_status *st = nullptr;        // host-memory calls
    unsigned long long *pw = nullptr;    // host-memory calls: [S][T + 1]
  } d;
};

namespace {

int make_device(kq_tone_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots, T = (size_t)b->g.T;
  if (d.slots.alloc(*b, S) || kq::tonecorr::alloc_table(*b, &d.table) || b->alloc(&d.incs, T) || b->alloc(&d.state, S, true) ||
      b->alloc(&d.acc, S * (2 * T + 1), true) || b->alloc(&d.last, S * T, true) ||
      d.arena.alloc(*b, S, b->cfg.max_events))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.incs, b->incs.data(), T * sizeof(unsigned), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// zero sums, powers, counters and arena, no run open (the stream is idle: callers synchronised it)
int cold_start(kq_tone_bank *b, unsigned s) {
  size_t const T = (size_t)b->g.T;
  static ToneState const init = [] {
    ToneState i{};
    i.cur = -1;
    return i;
  }();
  KQ_TRY(hipMemcpyAsync(b->d.state + s, &init, sizeof init, hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipMemsetAsync(b->d.acc + s * (2 * T + 1), 0, (2 * T + 1) * sizeof(long long), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.last + s * T, 0, T * sizeof(unsigned long long), b->stream));
  return b->d.arena.clear(*b, s, 1);
}

}  // namespace

extern "C" {

kq_tone_bank *kq_tone_create(const kq_tone_config *cfg) {
  const char *fn = "kq_tone_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  double const Fs = cfg->samprate;
  if (!kq::samprate_ok(fn, Fs) || !kq::field_in_range(fn, "block_len", cfg->block_len, 8, 4096) ||
      !kq::field_in_range(fn, "ntones", cfg->ntones, 1, kMaxTones))
    return nullptr;
  if (cfg->group0 == 0 || (uint64_t)cfg->group0 + cfg->group1 != cfg->ntones) {
    kq_internal_set_error("%s: groups of %u and %u tones must be one or two that are not empty and cover ntones %u", fn,
                          cfg->group0, cfg->group1, cfg->ntones);
    return nullptr;
  }
  if (!cfg->freqs) {
    kq_internal_set_error("%s: null freqs", fn);
    return nullptr;
  }
  for (unsigned t = 0; t < cfg->ntones; t++) {
    double const f = cfg->freqs[t];
    if (!(f > 0) || !(f < 0.5 * Fs)) {
      kq_internal_set_error("%s: freqs[%u] %g must be above 0 and below samprate / 2", fn, t, f);
      return nullptr;
    }
  }
  if (!kq::field_in_range(fn, "frac", cfg->frac, 1, 128) || !kq::field_in_range(fn, "ratio", cfg->ratio, 16, 4095) ||
      !kq::field_in_range(fn, "twist", cfg->twist, 16, 4095) || !kq::field_in_range(fn, "min_blocks", cfg->min_blocks, 1, 65535) ||
      !kq::input_scale_ok(fn, cfg->input_scale) || !kq::field_in_range(fn, "max_slots", cfg->max_slots, 1, kMaxSlots) ||
      !kq::field_in_range(fn, "max_events", cfg->max_events, 1, 4096) || !kq::max_samples_ok(fn, cfg->max_samples))
    return nullptr;
  (void)kq::tonecorr::cos_table();  // the table exists from here on
  kq_tone_bank *b = new kq_tone_bank;
  b->cfg = *cfg;
  b->freqs.assign(cfg->freqs, cfg->freqs + cfg->ntones);
  b->cfg.freqs = b->freqs.data();
  for (float f : b->freqs) b->incs.push_back((unsigned)std::llrint((double)f * 4294967296.0 / Fs));
  ToneGeom &g = b->g;
  g.B = (int)cfg->block_len;
  g.T = (int)cfg->ntones;
  g.Tpad = 1;
  while (g.Tpad < g.T) g.Tpad <<= 1;
  g.g0 = (int)cfg->group0;
  g.g1 = (int)cfg->group1;
  g.min_e = (unsigned long long)cfg->min_ms * cfg->block_len;
  g.frac = cfg->frac;
  g.ratio = cfg->ratio;
  g.twist = cfg->twist;
  g.min_blocks = cfg->min_blocks;
  g.max_events = (int)cfg->max_events;
  return b;
}

int kq_tone_destroy(kq_tone_bank *b) { return kq::destroy_bank(b, "kq_tone_destroy"); }

int kq_tone_set(kq_tone_bank *b, unsigned slot, const kq_tone_params *p) {
  if (!kq::set_args_ok("kq_tone_set", slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("kq_tone_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("kq_tone_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  TonePar np{};
  np.active = 1;
  np.source = p->source;
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_tone_remove(kq_tone_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_tone_remove"); }

int kq_tone_process(kq_tone_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_tone_status *status, size_t status_stride, uint64_t *powers,
                    size_t powers_stride) {
  const char *fn = "kq_tone_process";
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::call_args_ok(fn, format, b->cfg.max_samples, row_stride, block_len, nblocks, status, status_stride)) return -1;
  size_t const ncall = (size_t)block_len * nblocks, T = (size_t)b->g.T;
  if (powers && powers_stride < T + 1) {
    kq_internal_set_error("%s: powers_stride %zu < ntones + 1 = %zu", fn, powers_stride, T + 1);
    return -1;
  }
  std::optional<kq::DeviceScope> scope;
  kq::CallWork const work = kq::begin_call(b, fn, ncall, src, scope);
  if (work != kq::CALL_RUN) return work == kq::CALL_FAILED ? -1 : 0;
  auto &d = b->d;
  size_t const S = b->cfg.max_slots, nlist = d.slots.all.size();
  CallArgs a{};
  a.g = b->g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.table = d.table;
  a.incs = d.incs;
  a.state = d.state;
  a.acc = d.acc;
  a.last = d.last;
  a.ev = d.arena.ev;
  a.nev = d.arena.n;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  if (kq::bind_pcm(&a.in, &a.rowmap, *b, d.slots, b->cfg.max_samples, b->cfg.input_scale, src, format, src_stride, row_stride, block_len,
                   nblocks, on_device) ||
      kq::bind_status(b, on_device, status, status_stride, &a.st, &a.sstride))
    return -1;
  if (!on_device && powers && !d.pw && b->alloc(&d.pw, S * (T + 1))) return -1;
  a.pw = on_device || !powers ? reinterpret_cast<unsigned long long *>(powers) : d.pw;
  a.pstride = on_device ? powers_stride : T + 1;
  hipLaunchKernelGGL(k_tone, dim3((unsigned)nlist), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  if (on_device) return 0;
  return kq::end_host_call(b, status, status_stride, [&](size_t s0, size_t n) {  // the powers ride with the records
    return powers ? kq::copy_rows_back(*b, powers, powers_stride, d.pw, T + 1, T + 1, sizeof(uint64_t), s0, n) : 0;
  });
}

int kq_tone_pull_counts(kq_tone_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_tone_pull_counts", counts); }

int kq_tone_pull_event(kq_tone_bank *b, unsigned slot, unsigned index, kq_tone_event *event) {
  return kq::pull_event(b, "kq_tone_pull_event", slot, index, event);
}

int kq_tone_clear_events(kq_tone_bank *b) { return kq::clear_arena(b, "kq_tone_clear_events"); }

int kq_tone_get_table(const kq_tone_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_tone_get_table", dst, cap);
}

int kq_tone_get_incs(const kq_tone_bank *b, uint32_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_tone_get_incs: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_tone_get_incs: null dst");
    return -1;
  }
  size_t const n = std::min(cap, b->incs.size());
  if (n) std::memcpy(dst, b->incs.data(), n * sizeof(uint32_t));
  return (int)b->incs.size();
}

int kq_tone_sync(kq_tone_bank *b) { return kq::sync_bank(b, "kq_tone_sync"); }

int kq_tone_reset(kq_tone_bank *b) {
  return kq::reset_slots(b, "kq_tone_reset", [b](unsigned s) { return cold_start(b, s); });
}

}  // extern "C"
