// kq_cw.hip -- CW (Morse) decoder bank: the audio of CW channels -> characters, as events (code, elements, dot length,
// start, end, peak) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_cw_*): quantise as kq_tone_*, correlate every frame of B samples against one tone from
// the 1024-entry cosine table with a phase that is a function of the sample index alone, and step the tracker (peak,
// floor, threshold with hysteresis, debounce, dot-length tracking, character and word gaps) once per completed frame.  All
// exact integers after the quantiser.  State on the device, per slot: one kq_cw_status record (the open frame's I and Q
// and the whole tracker) and the arena of events; per bank the table.
//
// k_cw  one wave per slot, four slots to a workgroup.  A slot has one tone and frames of a few dozen samples, so a
//       workgroup per slot (k_tone) would leave most of its lanes without work.  The call's samples go through LDS once, a
//       piece of 64 / L frames at a time, quantised as they are loaded (coalesced: lane i takes samples i, i + 64, ...),
//       each frame at a stride Bs >= B with Bs / 2 odd, so that lanes reading sample i of 32 consecutive frames hit 32
//       banks.  Lane (f, p) of 64 / L x L takes samples p, p + L, ... of frame f against the table (cosine and sine packed
//       in one LDS word), two 64-bit multiply-adds a sample; its phase comes from the sample index.  L = 1 where 64 frames
//       fit the piece and the call has that many: then no lane ever talks to another.  Otherwise the L partial sums of a
//       frame are folded by shuffles; the sums are exact, so L changes no result, and the host picks it per call: the
//       least that fits the piece, and more where the call has too few frames to fill the wave.  The frame leaders
//       square into LDS and lane 0 walks the piece's P values in order through the tracker; the other waves of the
//       workgroup meet it at the next barrier (every wave has the same pieces: the frame grid is shared).  The carried
//       record is read once and written once per call.  No atomics, no scratch.
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

using kq::tonecorr::kTable;
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

struct CallArgs {
  CwGeom g;
  const CwPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;            // [1024]
  kq_cw_status *state;           // [S]
  kq_cw_event *ev;               // [S][max_events]
  unsigned *nev;                 // [S]
  int nlist;
  int L;                         // lanes to a frame, a power of two <= 64
  int64_t n0, n1;                // the call's samples
  kq::PcmIn in;
  // output
  kq_cw_status *st;
  size_t sstride;
};

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
  if (s.frames != 0xFFFFFFFFu) s.frames++;
  if (P > s.hi)
    s.hi = P;
  else
    s.hi -= s.hi >> 8;
  bool const valid = s.frames >= g.warm && s.hi >= g.min_p && s.hi >= (s.lo >> 4) * g.snr;
  unsigned long long const d = s.hi > s.lo ? s.hi - s.lo : 0;
  unsigned long long const thr = s.lo + (s.key ? d >> 3 : d >> 2);
  unsigned const lev = valid && P >= thr ? 1u : 0u;
  if (lev == 0 || (s.key && 16ull * s.run > 8ull * s.unit)) s.lo = (unsigned long long)((long long)s.lo + (((long long)P - (long long)s.lo) >> 5));
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
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * kWaves + wave;
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  kq::tonecorr::load_packed_table(CS, c.table, tid, kThreads);
  CwPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const B = g.grid.B, L = c.L, F = 64 / L, f = lane / L, p = lane & (L - 1);
  unsigned const inc[1] = {par.inc};
  // carried: lane 0 holds the record, the open frame's I and Q in it
  kq_cw_status s{};
  unsigned nev = 0;
  kq_cw_event *ev = c.ev + (size_t)slot * g.max_events;
  if (live && lane == 0) {
    s = c.state[slot];
    nev = c.nev[slot];
  }
  long long cy[2] = {s.acc_i, s.acc_q};
  int64_t n = c.n0, k0 = c.n0 / B;
  while (n < c.n1) {  // one piece: the frames k0 .. k0 + F - 1, from n to their end or the call's; x counts from k0 B
    int64_t const pe = (k0 + F) * (int64_t)B, e = pe < c.n1 ? pe : c.n1;
    int const x0 = (int)(n - k0 * B), x1 = x0 + (int)(e - n);  // x1 <= F B
    long long sm[2];  // (its first barrier: the piece before is done with q, Pb and carry)
    kq::tonecorr::correlate_piece<1>(g.grid, c.in, row, live, lane, L, c.n0, n, k0, x0, x1, qs[wave], CS, inc, sm, cy);
    int const done = (int)__umulhi((unsigned)x1, g.grid.magic);  // frames of the piece that are complete
    if (p == 0 && f * B < x1) {
      if (f < done) {
        long long const a = sm[0] >> 15, b = sm[1] >> 15;
        Pb[wave][f] = (unsigned long long)(a * a) + (unsigned long long)(b * b);
      } else {  // the call ends inside frame f
        carry[wave][0] = sm[0];
        carry[wave][1] = sm[1];
      }
    }
    __syncthreads();
    if (live && lane == 0) {
      for (int i = 0; i < done; i++) track(g, s, Pb[wave][i], (unsigned long long)(k0 + i), ev, nev);
      if (done * B < x1) {
        cy[0] = carry[wave][0];
        cy[1] = carry[wave][1];
      }
    }
    n = e;
    k0 += F;
  }
  if (live && lane == 0) {
    s.acc_i = cy[0];
    s.acc_q = cy[1];
    c.state[slot] = s;
    c.nev[slot] = nev;
    if (c.st) c.st[(size_t)slot * c.sstride] = s;
  }
}

// the dot of `wpm` in sixteenths of a frame
double unit_of(double Fs, unsigned B, float wpm) { return 19.2 * Fs / ((double)B * (double)wpm); }

}  // namespace

struct kq_cw_bank : kq::HostSide {
  static constexpr bool kDeferred = true;
  kq_cw_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  CwGeom g{};
  int Lmin = 1;                  // the least lanes to a frame whose piece fits kTile
  uint64_t n_cur = 0;
  kq::DeferredSlots<CwPar> def;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<CwPar> slots;
    short *table = nullptr;
    kq_cw_status *state = nullptr;
    kq::EventArena<kq_cw_event> arena;
    kq_cw_status *st = nullptr;          // host-memory calls
  } d;

  int to_device();
};

namespace {

int make_device(kq_cw_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots;
  if (d.slots.alloc(*b, S) || kq::tonecorr::alloc_table(*b, &d.table) || b->alloc(&d.state, S, true) ||
      d.arena.alloc(*b, S, b->cfg.max_events))
    return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // namespace

// kq::DeferredSlots::flush; the record of a slot that is set starts cold (the header's state at the set: its own u0, an
// empty character, both gaps reported) and its arena empty
int kq_cw_bank::to_device() {
  std::vector<kq_cw_status> cold(def.dirty.size());  // all zero; a run's records are copied from here
  size_t used = 0;
  return def.flush(this, make_device, [&](size_t s0, size_t n) {
    kq_cw_status *r = cold.data() + used;
    used += n;
    for (size_t i = 0; i < n; i++) {
      r[i].unit = d.slots.par[s0 + i].u0;
      r[i].code = 1;
      r[i].flags = 3;
    }
    KQ_TRY(hipMemcpyAsync(d.state + s0, r, n * sizeof *r, hipMemcpyHostToDevice, stream));
    return d.arena.clear(*this, s0, n);
  });
}

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
  (void)kq::tonecorr::cos_table();  // the table exists from here on
  kq_cw_bank *b = new kq_cw_bank;
  b->cfg = *cfg;
  b->def.init(cfg->max_slots);
  CwGeom &g = b->g;
  g.grid = kq::tonecorr::frame_grid(cfg->block_len);
  g.deb = cfg->deb;
  g.warm = cfg->warm;
  g.snr = cfg->snr;
  g.u_min = (unsigned)lo;
  g.u_max = (unsigned)hi;
  g.min_p = cfg->min_p;
  g.max_events = (int)cfg->max_events;
  b->Lmin = kq::tonecorr::least_lanes(g.grid, kTile);  // 64 at the most: Bs <= 4098
  return b;
}

int kq_cw_destroy(kq_cw_bank *b) { return kq::destroy_bank(b, "kq_cw_destroy"); }

int kq_cw_set(kq_cw_bank *b, unsigned slot, const kq_cw_params *p) {
  const char *fn = "kq_cw_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  double const Fs = b->cfg.samprate, f = p->pitch;
  if (!(f > 0) || !(f < 0.5 * Fs)) {
    kq_internal_set_error("%s: pitch %g must be above 0 and below samprate / 2", fn, f);
    return -1;
  }
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
  const char *fn = "kq_cw_process";
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::call_args_ok(fn, format, b->cfg.max_samples, row_stride, block_len, nblocks, status, status_stride)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  std::optional<kq::DeviceScope> scope;
  kq::CallWork const work = kq::begin_call(b, fn, ncall, src, scope);
  if (work != kq::CALL_RUN) return work == kq::CALL_FAILED ? -1 : 0;
  auto &d = b->d;
  size_t const nlist = d.slots.all.size();
  CallArgs a{};
  a.g = b->g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.table = d.table;
  a.state = d.state;
  a.ev = d.arena.ev;
  a.nev = d.arena.n;
  a.nlist = (int)nlist;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  a.L = kq::tonecorr::lanes_for_call(b->g.grid, b->Lmin, ncall);
  if (kq::bind_pcm(&a.in, &a.rowmap, *b, d.slots, b->cfg.max_samples, b->cfg.input_scale, src, format, src_stride, row_stride, block_len,
                   nblocks, on_device) ||
      kq::bind_status(b, on_device, status, status_stride, &a.st, &a.sstride))
    return -1;
  hipLaunchKernelGGL(k_cw, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_cw_pull_counts(kq_cw_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_cw_pull_counts", counts); }

int kq_cw_pull_event(kq_cw_bank *b, unsigned slot, unsigned index, kq_cw_event *event) {
  return kq::pull_event(b, "kq_cw_pull_event", slot, index, event);
}

int kq_cw_clear_events(kq_cw_bank *b) { return kq::clear_arena(b, "kq_cw_clear_events"); }

int kq_cw_get_table(const kq_cw_bank *b, int16_t *dst, size_t cap) { return kq::tonecorr::get_table(b, "kq_cw_get_table", dst, cap); }

int kq_cw_get_inc(kq_cw_bank *b, unsigned slot, uint32_t *inc) {
  if (!b) {
    kq_internal_set_error("kq_cw_get_inc: null bank");
    return -1;
  }
  if (!inc) {
    kq_internal_set_error("kq_cw_get_inc: null inc");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("kq_cw_get_inc: slot %u holds no decoder", slot);
    return -1;
  }
  *inc = b->def.want[slot].inc;
  return 0;
}

int kq_cw_sync(kq_cw_bank *b) { return kq::sync_bank(b, "kq_cw_sync"); }

int kq_cw_reset(kq_cw_bank *b) { return kq::deferred_reset(b, "kq_cw_reset"); }

}  // extern "C"
