// kq_cw.hip -- CW (Morse) decoder bank: the audio of CW channels -> characters, as events (code, elements, dot length,
// start, end, peak) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_cw_*): quantise as kq_tone_*, correlate every frame of B samples against one tone from
// the 1024-entry cosine table with a phase that is a function of the sample index alone, and step the tracker (peak,
// floor, threshold with hysteresis, debounce, dot-length tracking, character and word gaps) once per completed frame.  All
// exact integers after the quantiser.  State on the device, per slot: one kq_cw_status record (the open frame's I and Q
// and the whole tracker) and the arena of events; per bank the table.
//
// k_cw  a frame-grid kernel without a window (kq_tonecorr.hpp describes the mapping): one tone.  The frame leaders square
//       into LDS and lane 0 walks the piece's P values in order through the tracker.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <mutex>

#include "ka9q_hip.h"
#include "kq_tonecorr.hpp"

namespace tc = kq::tonecorr;

namespace {

using tc::kTable;
constexpr unsigned kMaxSlots = 16384;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 4288;                     // samples a wave keeps in LDS: 64 frames of B = 64 at stride 66, and a few more
constexpr unsigned kRunMax = 0x0FFFFFFFu;

struct CwGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned deb, warm, snr, u_min, u_max;
  unsigned long long min_p;
  int max_events;
};

struct CwPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc, u0;
};

struct CwKind {
  using Config = kq_cw_config;
  using Geom = CwGeom;
  using Par = CwPar;
  using Status = kq_cw_status;
  using Event = kq_cw_event;
  using Hist = void;
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = false;
  // the header's state at the set: the slot's own u0, an empty character, both gaps reported
  static void cold(CwPar const &p, kq_cw_status &r) {
    r.unit = p.u0;
    r.code = 1;
    r.flags = 3;
  }
};
using CallArgs = tc::GridBank<CwKind>::Args;

__device__ __forceinline__ void file_event(CwGeom const &g, kq_cw_status &s, unsigned code, unsigned nelem,
                                           unsigned long long start, unsigned long long end, kq_cw_event *ev, unsigned &nev) {
  s.events++;
  if (nev >= (unsigned)g.max_events) {
    s.dropped++;
    return;
  }
  kq_cw_event r;
  r.code = code;
  r.nelem = nelem;
  r.unit = s.unit;
  r.reserved = 0;
  r.start_sample = start * (unsigned long long)g.grid.B;
  r.end_sample = end * (unsigned long long)g.grid.B;
  r.peak = s.hi;
  ev[nev++] = r;
}

// the header's step 6: a mark of `run` frames closes
__device__ __forceinline__ void close_mark(CwGeom const &g, kq_cw_status &s, unsigned run) {
  int const m = (int)(16u * run);  // run < 2^28
  int u = (int)s.unit;             // <= 2^20
  if (m > 8 * u) {
    s.code = 0;
  } else if (m < 2 * u) {
    s.code = 2 * s.code;
    u += (m - u) >> 2;
  } else {
    s.code = 2 * s.code + (s.code ? 1u : 0u);
    u += (m / 3 - u) >> 2;
  }
  s.unit = (unsigned)min(max(u, (int)g.u_min), (int)g.u_max);
  s.nelem++;
  if (s.nelem > 8) s.code = 0;
  s.flags = 0;
}

// the header's tracker: frame k with power P
__device__ __forceinline__ void track(CwGeom const &g, kq_cw_status &s, unsigned long long P, unsigned long long k,
                                      kq_cw_event *ev, unsigned &nev) {
  s.frames = tc::sat_inc(s.frames);
  if (P > s.hi)
    s.hi = P;
  else
    s.hi -= s.hi >> 8;
  bool const valid = s.frames >= g.warm && s.hi >= g.min_p && s.hi >= (s.lo >> 4) * g.snr;
  unsigned long long const d = s.hi > s.lo ? s.hi - s.lo : 0;
  unsigned long long const thr = s.lo + (s.key ? d >> 3 : d >> 2);
  unsigned const lev = valid && P >= thr ? 1u : 0u;
  if (lev == 0 || (s.key && 16ull * s.run > 8ull * s.unit)) tc::smooth(s.lo, P, 5);
  if (lev == s.key) {
    s.run = min(s.run + 1 + s.cand, kRunMax);
    s.cand = 0;
  } else {
    s.cand++;
    if (s.cand >= g.deb) {
      if (s.key) {
        close_mark(g, s, s.run);
        s.last = k + 1 - s.cand;
      } else if (s.nelem == 0) {
        s.first = k + 1 - s.cand;
      }
      s.key = lev;
      s.run = s.cand;
      s.cand = 0;
    }
  }
  if (!s.key) {
    if (!(s.flags & 1) && 16ull * s.run >= 2ull * s.unit) {
      file_event(g, s, s.code, s.nelem, s.first, s.last, ev, nev);
      s.code = 1;
      s.nelem = 0;
      s.flags |= 1;
    }
    if (!(s.flags & 2) && 16ull * s.run >= 5ull * s.unit) {
      file_event(g, s, 1, 0, s.last, k + 1, ev, nev);
      s.flags |= 2;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_cw(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ unsigned long long Pb[kWaves][64];
  __shared__ long long carry[kWaves][2];
  CwGeom const &g = c.g;
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane;
  unsigned const inc[1] = {w.par.inc};
  kq_cw_status s{};
  unsigned nev = 0;
  kq_cw_event *ev = tc::load_record(c, w, s, nev);
  long long cy[2] = {s.acc_i, s.acc_q};
  for (tc::Piece pc(c.n0, w.B); pc.n < c.n1; pc.next(w.F)) {
    pc.span(c.n1, w.B, w.F);
    long long sm[2];  // (its first barrier: the piece before is done with q, Pb and carry)
    tc::correlate_piece<1>(c, w, pc, qs[wave], CS, inc, sm, cy);
    int const done = pc.done(g.grid);
    if (w.p == 0 && w.f * w.B < pc.x1) {
      if (w.f < done) {
        long long const a = sm[0] >> 15, b = sm[1] >> 15;
        Pb[wave][w.f] = (unsigned long long)(a * a) + (unsigned long long)(b * b);
      } else {  // the call ends inside frame f
        carry[wave][0] = sm[0];
        carry[wave][1] = sm[1];
      }
    }
    __syncthreads();
    if (w.live && lane == 0) {
      for (int i = 0; i < done; i++) track(g, s, Pb[wave][i], (unsigned long long)(pc.k0 + i), ev, nev);
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  s.acc_i = cy[0];
  s.acc_q = cy[1];
  tc::store_record(c, w, s, nev);
}

// the dot of `wpm` in sixteenths of a frame
double unit_of(double Fs, unsigned B, float wpm) { return 19.2 * Fs / ((double)B * (double)wpm); }

}  // namespace

struct kq_cw_bank : tc::GridBank<CwKind> {};

extern "C" {

kq_cw_bank *kq_cw_create(const kq_cw_config *cfg) {
  const char *fn = "kq_cw_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  double const Fs = cfg->samprate;
  if (!kq::samprate_ok(fn, Fs) || !kq::field_in_range(fn, "block_len", cfg->block_len, 8, 4096)) return nullptr;
  if (!(cfg->min_wpm > 0) || !std::isfinite(cfg->max_wpm) || !(cfg->min_wpm <= cfg->max_wpm)) {
    kq_internal_set_error("%s: speeds %g..%g WPM must be positive, finite and in order", fn, (double)cfg->min_wpm,
                          (double)cfg->max_wpm);
    return nullptr;
  }
  double const lo = std::floor(unit_of(Fs, cfg->block_len, cfg->max_wpm)), hi = std::ceil(unit_of(Fs, cfg->block_len, cfg->min_wpm));
  if (!(lo >= 48.0)) {
    kq_internal_set_error("%s: max_wpm %g leaves a dot %g sixteenths of a frame of %u samples, fewer than 48 (3 frames)", fn,
                          (double)cfg->max_wpm, lo, cfg->block_len);
    return nullptr;
  }
  if (!(hi <= 1048576.0)) {
    kq_internal_set_error("%s: min_wpm %g makes a dot %g sixteenths of a frame of %u samples, more than 2^20", fn,
                          (double)cfg->min_wpm, hi, cfg->block_len);
    return nullptr;
  }
  if (!kq::field_in_range(fn, "deb", cfg->deb, 1, 16) || !kq::field_in_range(fn, "warm", cfg->warm, 0, 65535) ||
      !kq::field_in_range(fn, "snr", cfg->snr, 16, 4095) || !kq::min_p_ok(fn, cfg->min_p) ||
      !kq::input_scale_ok(fn, cfg->input_scale) || !kq::field_in_range(fn, "max_slots", cfg->max_slots, 1, kMaxSlots) ||
      !kq::field_in_range(fn, "max_events", cfg->max_events, 1, 4096) || !kq::max_samples_ok(fn, cfg->max_samples))
    return nullptr;
  kq_cw_bank *b = tc::finish_create<kq_cw_bank>(cfg, kTile);  // Lmin 64 at the most: Bs <= 4098
  b->g.deb = cfg->deb;
  b->g.u_min = (unsigned)lo;
  b->g.u_max = (unsigned)hi;
  return b;
}

int kq_cw_destroy(kq_cw_bank *b) { return kq::destroy_bank(b, "kq_cw_destroy"); }

int kq_cw_set(kq_cw_bank *b, unsigned slot, const kq_cw_params *p) {
  const char *fn = "kq_cw_set";
  std::unique_lock<std::mutex> lk;
  if (!tc::open_set(b, fn, slot, p, kMaxSlots, lk)) return -1;
  double const Fs = b->cfg.samprate, f = p->pitch;
  if (!tc::tone_ok(fn, Fs, f, "pitch %g", f)) return -1;
  if (!(p->wpm >= b->cfg.min_wpm) || !(p->wpm <= b->cfg.max_wpm)) {
    kq_internal_set_error("%s: wpm %g must be within the bank's %g..%g", fn, (double)p->wpm, (double)b->cfg.min_wpm,
                          (double)b->cfg.max_wpm);
    return -1;
  }
  CwPar np{};
  np.active = 1;
  np.source = p->source;
  np.inc = (unsigned)std::llrint(f * 4294967296.0 / Fs);
  np.u0 = std::min(std::max((unsigned)std::llrint(unit_of(Fs, b->cfg.block_len, p->wpm)), b->g.u_min), b->g.u_max);
  b->def.set(slot, np);
  return 0;
}

int kq_cw_remove(kq_cw_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_cw_remove"); }

int kq_cw_process(kq_cw_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                  unsigned nblocks, int on_device, kq_cw_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_cw_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL(k_cw, dim3(blocks), dim3(kThreads), 0, b->stream, a);
                               });
}

int kq_cw_pull_counts(kq_cw_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_cw_pull_counts", counts); }

int kq_cw_pull_event(kq_cw_bank *b, unsigned slot, unsigned index, kq_cw_event *event) {
  return kq::pull_event(b, "kq_cw_pull_event", slot, index, event);
}

int kq_cw_clear_events(kq_cw_bank *b) { return kq::clear_arena(b, "kq_cw_clear_events"); }

int kq_cw_get_table(const kq_cw_bank *b, int16_t *dst, size_t cap) { return kq::tonecorr::get_table(b, "kq_cw_get_table", dst, cap); }

int kq_cw_get_inc(kq_cw_bank *b, unsigned slot, uint32_t *inc) {
  std::unique_lock<std::mutex> lk;
  const CwPar *w = tc::wanted(b, "kq_cw_get_inc", slot, inc, "inc", lk);
  if (!w) return -1;
  *inc = w->inc;
  return 0;
}

int kq_cw_sync(kq_cw_bank *b) { return kq::sync_bank(b, "kq_cw_sync"); }

int kq_cw_reset(kq_cw_bank *b) { return kq::deferred_reset(b, "kq_cw_reset"); }

}  // extern "C"
