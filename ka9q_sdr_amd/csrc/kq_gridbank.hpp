// kq_gridbank.hpp -- the host half that the frame-grid decoders share (kq_cw, kq_rtty, kq_psk, kq_ale, kq_dsc, kq_navtex,
// kq_same), on top of kq_slots.hpp: deferred event banks of PCM decoders whose kernels correlate frames of B samples on a
// grid that starts at sample 0 of the stream (the device half: kq_tonecorr.hpp, which includes this file).  Host only, so
// that it compiles against the device-less stand-in for the runtime; the launch stays with each bank.
//
//   cos_table      C[j] = rint(32767 cos(2 pi j / 1024)), one instance for the library, for every bank that correlates
//                  against it (kq_tone and kq_acars too): alloc_table, its device copy; get_table, the body of kq_*_get_table
//   FrameGrid      frames of B samples, each at a stride Bs >= B in LDS with Bs / 2 odd, so that lanes reading sample i of 32
//                  consecutive frames hit 32 banks; the choice of L, the lanes to a frame, per bank (least_lanes) and per
//                  call (lanes_for_call)
//   FrameHist      the reduced sums of a slot's last 31 frames, as the device keeps them between calls
//   GridArgs       the fields every kernel's argument block begins with
//   GridBank<K>    the bank: its struct, make_device and to_device.  K names the bank's types and its two hooks:
//                    Config, Geom, Par, Status, Event   the public config, status and event; the kernels' geometry (with
//                                                       grid, warm, snr, min_p, max_events) and per-slot record
//                    Hist                               FrameHist<NS>, or void where the bank slides no window (kq_cw)
//                    Tables                             the bank's own device tables (NoTables; kq_ale's Golay tables)
//                    kZeroCold, cold(par, status &)     a set slot's record starts all zero, or as cold() fills it (kq_cw)
//                  A set slot's history starts all zero and its arena empty.
//   config_head_ok, config_tail_ok   the config checks that kq_{rtty,psk,ale,dsc}_create report first and last, in their order
//   finish_create  the tail of kq_*_create, behind the bank's checks
//   open_set, tone_ok, tone_pair, symbol_period, wanted, get_pair_slot, process   the shared parts of kq_*_set, the opening
//                  of a getter, a two-tone getter's assignments, and the body of kq_*_process around the bank's launch
//   PairPar, set_pair, get_pair   a slot that is a tone pair and a bit rate (kq_dsc, kq_navtex, kq_same): its record and the
//                  whole bodies of kq_*_set and kq_*_get_slot
//
// What a bank still writes: its K, Geom, Par and CallArgs; the checks of create in the order it reports them and the
// fields of Geom that are its own; the checks of set that are its own and the slot's record; the getters' assignments; the
// launch; the extern "C" one-liners.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "ka9q_hip.h"
#include "kq_host.hpp"
#include "kq_slots.hpp"

namespace kq {
namespace tonecorr {

constexpr int kTable = 1024;

// made once, at the first kq_*_create of any of the banks
inline std::vector<short> const &cos_table() {
  static std::vector<short> const table = [] {
    std::vector<short> t((size_t)kTable);
    for (int j = 0; j < kTable; j++) t[j] = (short)std::lrint(32767.0 * std::cos(2.0 * M_PI * j / kTable));
    return t;
  }();
  return table;
}

// the table on the device (queued: the caller waits)
inline int alloc_table(HostSide &h, short **table) {
  if (h.alloc(table, (size_t)kTable)) return -1;
  KQ_TRY(hipMemcpyAsync(*table, cos_table().data(), kTable * sizeof(short), hipMemcpyHostToDevice, h.stream));
  return 0;
}

// kq_*_get_table
inline int get_table(const void *b, const char *fn, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("%s: null dst", fn);
    return -1;
  }
  size_t const n = std::min(cap, (size_t)kTable);
  if (n) std::memcpy(dst, cos_table().data(), n * sizeof(int16_t));
  return kTable;
}

struct FrameGrid {
  int B, Bs;       // Bs: a frame's stride in LDS, >= B, Bs / 2 odd
  unsigned magic;  // ceil(2^32 / B): x / B = umulhi(x, magic) for x < 2^16
};

inline FrameGrid frame_grid(unsigned block_len) {
  FrameGrid g;
  g.B = (int)block_len;
  g.Bs = g.B + ((g.B & 1) ? 1 : 0);  // even
  if ((g.Bs & 3) == 0) g.Bs += 2;    // and Bs / 2 odd
  g.magic = (unsigned)((0x100000000ull + block_len - 1) / block_len);
  return g;
}

// the least lanes to a frame with which a piece, 64 / L frames, fits `tile` samples of LDS (64 at the latest where Bs <= tile)
inline int least_lanes(FrameGrid const &g, int tile) {
  int L = 1;
  while ((64 / L) * g.Bs > tile) L *= 2;
  return L;
}

// lanes to a frame for a call of ncall samples: what the piece needs, and more where the call's frames (at most nf) do not
// fill a wave.  The sums are exact, so L changes no result.
inline int lanes_for_call(FrameGrid const &g, int Lmin, size_t ncall) {
  size_t const nf = (ncall + (size_t)g.B - 2) / (size_t)g.B + 1;
  int L = Lmin;
  while (L < 64 && (size_t)(2 * L) * nf <= 64) L *= 2;
  return L;
}

constexpr int kHist = 31;  // frames of history a slot carries: W - 1 at the most

template <int NS>
struct FrameHist {
  int v[NS][kHist];  // a series to a row (I and Q of every tone); [kHist - 1] is the last completed frame
};

template <class Geom, class Par, class Status, class Event, class Hist>
struct GridArgs {
  Geom g;
  const Par *par;
  const int *list;      // active slots, ascending
  const int *rowmap;    // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;   // [1024]
  Status *state;        // [S]
  Hist *hist;           // [S] (void: the bank has none, and the pointer is null)
  Event *ev;            // [S][max_events]
  unsigned *nev;        // [S]
  int nlist;
  int L;                // lanes to a frame, a power of two <= 64
  int64_t n0, n1;       // the call's samples
  PcmIn in;
  // output
  Status *st;
  size_t sstride;
};

struct NoTables {
  int make(HostSide &) { return 0; }
};

template <class K>
struct GridBank : HostSide {
  using Par = typename K::Par;
  using Status = typename K::Status;
  using Hist = typename K::Hist;
  using Args = GridArgs<typename K::Geom, Par, Status, typename K::Event, Hist>;
  static constexpr bool kDeferred = true;
  typename K::Config cfg;
  std::mutex mu;
  bool dev_ready = false;
  typename K::Geom g{};
  int Lmin = 1;  // the least lanes to a frame whose piece fits the kernel's tile
  uint64_t n_cur = 0;
  DeferredSlots<Par> def;
  struct Dev {  // kq::lazy_device
    SlotTable<Par> slots;
    short *table = nullptr;
    typename K::Tables tables;
    Status *state = nullptr;
    Hist *hist = nullptr;
    EventArena<typename K::Event> arena;
    Status *st = nullptr;  // host-memory calls
  } d;

  int make_device() {
    if (open_stream(cfg.stream)) return -1;
    size_t const S = cfg.max_slots;
    if (d.slots.alloc(*this, S) || alloc_table(*this, &d.table) || d.tables.make(*this) || alloc(&d.state, S, true)) return -1;
    if constexpr (!std::is_void<Hist>::value)
      if (alloc(&d.hist, S, true)) return -1;
    if (d.arena.alloc(*this, S, cfg.max_events)) return -1;
    KQ_TRY(hipStreamSynchronize(stream));
    return 0;
  }

  // kq::DeferredSlots::flush with the cold start of a run of set slots: the records (the header's state at the set), the
  // history and the arena
  int to_device() {
    std::vector<Status> cold(K::kZeroCold ? 0 : def.dirty.size());  // all zero; a run's records are copied from here
    size_t used = 0;
    return def.flush(this, [](GridBank *b) { return b->make_device(); }, [&](size_t s0, size_t n) {
      if constexpr (K::kZeroCold) {
        KQ_TRY(hipMemsetAsync(d.state + s0, 0, n * sizeof(Status), stream));
      } else {
        Status *r = cold.data() + used;
        used += n;
        for (size_t i = 0; i < n; i++) K::cold(d.slots.par[s0 + i], r[i]);
        KQ_TRY(hipMemcpyAsync(d.state + s0, r, n * sizeof *r, hipMemcpyHostToDevice, stream));
      }
      if constexpr (!std::is_void<Hist>::value) KQ_TRY(hipMemsetAsync(d.hist + s0, 0, n * sizeof(Hist), stream));
      return d.arena.clear(*this, s0, n);
    });
  }
};

// The checks of kq_*_create that the banks with frames of 8..256 samples share (kq_cw has other limits and another order):
// the head, then the bank's own fields, then the tail.  Each reports the first field it refuses.
template <class Config>
bool config_head_ok(const char *fn, const Config *cfg) {
  return kq::samprate_ok(fn, cfg->samprate) && kq::field_in_range(fn, "block_len", cfg->block_len, 8, 256) &&
         kq::field_in_range(fn, "warm", cfg->warm, 0, 65535) && kq::field_in_range(fn, "snr", cfg->snr, 16, 4095) &&
         kq::min_p_ok(fn, cfg->min_p) && kq::input_scale_ok(fn, cfg->input_scale);
}

template <class Config>
bool config_tail_ok(const char *fn, const Config *cfg, unsigned slot_limit) {
  return kq::field_in_range(fn, "max_slots", cfg->max_slots, 1, slot_limit) &&
         kq::field_in_range(fn, "max_events", cfg->max_events, 1, 4096) && kq::max_samples_ok(fn, cfg->max_samples);
}

// the tail of kq_*_create, once the bank's checks have passed: the bank with its config, its slots, the grid and what every
// Geom has of the config; `tile`: the samples a wave of the bank's kernel keeps in LDS
template <class Bank, class Config>
Bank *finish_create(const Config *cfg, int tile) {
  (void)cos_table();  // the table exists from here on
  Bank *b = new Bank;
  b->cfg = *cfg;
  b->def.init(cfg->max_slots);
  b->g.grid = frame_grid(cfg->block_len);
  b->g.warm = cfg->warm;
  b->g.snr = cfg->snr;
  b->g.min_p = cfg->min_p;
  b->g.max_events = (int)cfg->max_events;
  b->Lmin = least_lanes(b->g.grid, tile);
  return b;
}

// The opening of kq_*_set: the slot against any bank's limit, the parameters and the bank there at all, the bank's lock
// taken into `lk`, the slot against this bank's.
template <class Bank>
bool open_set(Bank *b, const char *fn, unsigned slot, const void *params, unsigned slot_limit, std::unique_lock<std::mutex> &lk) {
  if (!set_args_ok(fn, slot, params, slot_limit)) return false;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return false;
  }
  lk = std::unique_lock<std::mutex>(b->mu);
  return slot_in_bank(fn, slot, b->cfg.max_slots);
}

// a tone at f against 0 < f < Fs / 2; `what` with its arguments, as for printf, says which tone and where in the error text
__attribute__((format(printf, 4, 5))) inline bool tone_ok(const char *fn, double Fs, double f, const char *what, ...) {
  if (f > 0 && f < 0.5 * Fs) return true;
  char name[160];
  va_list ap;
  va_start(ap, what);
  vsnprintf(name, sizeof name, what, ap);
  va_end(ap);
  kq_internal_set_error("%s: %s must be above 0 and below samprate / 2", fn, name);
  return false;
}

// a mark / space pair (kq_rtty, set_pair): both tones against 0 < f < Fs / 2 and against each other, then their phase
// increments, rint(f 2^32 / Fs) in double
inline bool tone_pair(const char *fn, double Fs, float mark, float space, unsigned *inc_m, unsigned *inc_s) {
  double const fm = mark, fs = space;
  if (!tone_ok(fn, Fs, fm, "mark %g", fm) || !tone_ok(fn, Fs, fs, "space %g", fs)) return false;
  if (mark == space) {
    kq_internal_set_error("%s: mark and space are both %g", fn, fm);
    return false;
  }
  *inc_m = (unsigned)std::llrint(fm * 4294967296.0 / Fs);
  *inc_s = (unsigned)std::llrint(fs * 4294967296.0 / Fs);
  return true;
}

// the period of a bit or symbol (`noun`) of `baud` in 1/256 frame, *tb = rint(256 Fs / (B baud)) within 2048..8192, and
// the window one period long in frames, *W
inline bool symbol_period(const char *fn, double Fs, unsigned B, double baud, const char *noun, int *tb, int *W) {
  if (!(baud > 0) || !std::isfinite(baud)) {
    kq_internal_set_error("%s: baud %g must be positive and finite", fn, baud);
    return false;
  }
  double const t = std::rint(256.0 * Fs / ((double)B * baud));
  if (!(t >= 2048.0) || !(t <= 8192.0)) {
    kq_internal_set_error("%s: baud %g makes tb %.10g, a %s of %g frames of %u samples, outside 2048..8192 (8 to 32 frames)", fn, baud,
                          t, noun, t / 256.0, B);
    return false;
  }
  *tb = (int)t;
  *W = (*tb + 128) >> 8;
  return true;
}

// The opening of a getter: the bank and `out` (`out_name`: the parameter's own name) there at all, the bank's lock taken
// into `lk`; the record of `slot` as it was last set, or null with the error text set
template <class Bank>
const typename Bank::Par *wanted(Bank *b, const char *fn, unsigned slot, const void *out, const char *out_name,
                                 std::unique_lock<std::mutex> &lk) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return nullptr;
  }
  if (!out) {
    kq_internal_set_error("%s: null %s", fn, out_name);
    return nullptr;
  }
  lk = std::unique_lock<std::mutex>(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("%s: slot %u holds no decoder", fn, slot);
    return nullptr;
  }
  return &b->def.want[slot];
}

// a two-tone slot's record as kq_*_get_slot hands it out: {inc_m, inc_s, tb, W}
template <class Par, class Slot>
void get_pair_slot(Par const &w, Slot *out) {
  out->inc_m = w.inc_m;
  out->inc_s = w.inc_s;
  out->tb = (uint32_t)w.tb;
  out->W = (uint32_t)w.W;
}

// The banks whose slot is a mark / space pair and a bit rate and nothing else (kq_dsc, kq_navtex, kq_same): the slot's
// record, and the bodies of kq_*_set and kq_*_get_slot
struct PairPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc_m, inc_s;
  int tb, W;
};

template <class Bank, class Params>
int set_pair(Bank *b, const char *fn, unsigned slot, const Params *p, unsigned slot_limit) {
  std::unique_lock<std::mutex> lk;
  if (!open_set(b, fn, slot, p, slot_limit, lk)) return -1;
  double const Fs = b->cfg.samprate;
  PairPar np{};
  if (!tone_pair(fn, Fs, p->mark, p->space, &np.inc_m, &np.inc_s) ||
      !symbol_period(fn, Fs, b->cfg.block_len, p->baud, "bit", &np.tb, &np.W))
    return -1;
  np.active = 1;
  np.source = p->source;
  b->def.set(slot, np);
  return 0;
}

template <class Bank, class Slot>
int get_pair(Bank *b, const char *fn, unsigned slot, Slot *out) {
  std::unique_lock<std::mutex> lk;
  const PairPar *w = wanted(b, fn, slot, out, "out", lk);
  if (!w) return -1;
  get_pair_slot(*w, out);
  return 0;
}

// The body of kq_*_process.  Args: the bank's argument block, Bank::Args or a struct on it; launch(args, blocks) fills what
// the block has beyond GridArgs and launches the kernel on the bank's stream, `waves` slots to a workgroup.
template <class Args, class Bank, class Launch>
int process(Bank *b, const char *fn, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
            unsigned nblocks, int on_device, typename Bank::Status *status, size_t status_stride, int waves, Launch launch) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!call_args_ok(fn, format, b->cfg.max_samples, row_stride, block_len, nblocks, status, status_stride)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  std::optional<DeviceScope> scope;
  CallWork const work = begin_call(b, fn, ncall, src, scope);
  if (work != CALL_RUN) return work == CALL_FAILED ? -1 : 0;
  auto &d = b->d;
  size_t const nlist = d.slots.all.size();
  Args a{};
  a.g = b->g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.table = d.table;
  a.state = d.state;
  a.hist = d.hist;
  a.ev = d.arena.ev;
  a.nev = d.arena.n;
  a.nlist = (int)nlist;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  a.L = lanes_for_call(b->g.grid, b->Lmin, ncall);
  if (bind_pcm(&a.in, &a.rowmap, *b, d.slots, b->cfg.max_samples, b->cfg.input_scale, src, format, src_stride, row_stride, block_len,
               nblocks, on_device) ||
      bind_status(b, on_device, status, status_stride, &a.st, &a.sstride))
    return -1;
  launch(a, (unsigned)((nlist + waves - 1) / waves));
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  return on_device ? 0 : end_host_call(b, status, status_stride, nullptr);
}

}  // namespace tonecorr
}  // namespace kq
