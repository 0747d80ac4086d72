// kq_rtty.hip -- RTTY (start-stop FSK teleprinter) decoder bank: the audio of SSB channels -> characters, as events (code,
// flags, start, sig, nse) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_rtty_*): quantise as kq_cw_*, correlate every frame of B samples against the mark and
// the space tone from the 1024-entry cosine table with phases that are functions of the sample index alone, slide a
// window one bit long (W frames) over the frames' reduced sums, and step the start-stop framer once per completed frame.
// All exact integers after the quantiser.  State on the device, per slot: one kq_rtty_status record (the open frame's I
// and Q of both tones, the window sums, the levels and the framer), the reduced sums of the last 31 frames, and the arena
// of events; per bank the table.
//
// k_rtty  k_cw's mapping: one wave per slot, four slots to a workgroup.  The call's samples go through LDS once, a piece of
//         64 / L frames at a time, quantised as they are loaded, each frame at a stride Bs >= B with Bs / 2 odd.  Lane
//         (f, p) of 64 / L x L takes samples p, p + L, ... of frame f and uses each for both tones: one sample read, two
//         packed table reads, four 64-bit multiply-adds.  The L partial sums of a frame are folded by shuffles; the sums
//         are exact, so L changes no result and the host picks it per call.  The frame leaders write the four reduced
//         sums to LDS behind the 31 carried frames of history (W <= 32), lane f then sums its own W entries per tone and
//         squares -- exact, so no scan order matters -- and lane 0 walks the piece's (Pm, Ps) pairs in order through the
//         levels and the framer.  The baud rate and W differ from slot to slot; B and the frame grid do not, so every wave
//         of a workgroup has the same pieces and the barriers are uniform.  The carried record and the history are read
//         once and written once per call.  No atomics, no scratch.
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
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50; with the rest
                                                // the workgroup stays under 40 KiB, four workgroups to a CU
constexpr int kHist = 31;                       // frames of history a slot carries: W - 1 at the most
constexpr int kRow = kHist + 64 + 1;            // a wave's reduced sums of one kind: the history and a piece's frames
constexpr unsigned kWait = 0, kIdle = 1, kChar = 2;

struct RttyGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr;
  unsigned long long min_p;
  int max_events;
};

struct RttyPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc_m, inc_s;
  int tb, W, nbits;
};

struct RttyHist {
  int v[4][kHist];               // a, b of mark, a, b of space; [kHist - 1] is the last completed frame
};

struct CallArgs {
  RttyGeom g;
  const RttyPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;            // [1024]
  kq_rtty_status *state;         // [S]
  RttyHist *hist;                // [S]
  kq_rtty_event *ev;             // [S][max_events]
  unsigned *nev;                 // [S]
  int nlist;
  int L;                         // lanes to a frame, a power of two <= 64
  int64_t n0, n1;                // the call's samples
  kq::PcmIn in;
  // output
  kq_rtty_status *st;
  size_t sstride;
};

__device__ __forceinline__ unsigned sat_inc(unsigned v) { return v == 0xFFFFFFFFu ? v : v + 1; }

__device__ __forceinline__ void file_event(RttyGeom const &g, kq_rtty_status &s, unsigned flags, kq_rtty_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_rtty_event r;
  r.code = s.code;
  r.flags = flags;
  r.start_sample = s.start * (unsigned long long)g.grid.B;
  r.sig = s.sig;
  r.nse = s.nse;
  ev[nev++] = r;
}

// the header's steps 1 to 4: frame k with the window's powers Pm and Ps
__device__ __forceinline__ void step(RttyGeom const &g, RttyPar const &par, kq_rtty_status &s, unsigned long long Pm,
                                     unsigned long long Ps, unsigned long long k, kq_rtty_event *ev, unsigned &nev) {
  s.frames = sat_inc(s.frames);
  unsigned long long const hi = Pm >= Ps ? Pm : Ps, lo = Pm >= Ps ? Ps : Pm;
  unsigned const lev = Pm >= Ps ? 1u : 0u;
  bool const samp = s.state == kChar && s.t - 256 < 128;
  if (s.state != kChar || samp) {  // every value is below 2^63: the differences fit
    int const sh = samp ? 4 : 6;
    s.sig = (unsigned long long)((long long)s.sig + (((long long)hi - (long long)s.sig) >> sh));
    s.nse = (unsigned long long)((long long)s.nse + (((long long)lo - (long long)s.nse) >> sh));
  }
  // 16 sig >= nse snr in 128 bits: (sig >> 60, sig << 4) against (umulhi(nse, snr), nse snr)
  unsigned long long const lh = s.sig >> 60, ll = s.sig << 4, rh = __umul64hi(s.nse, (unsigned long long)g.snr),
                           rl = s.nse * (unsigned long long)g.snr;
  bool const ratio = lh > rh || (lh == rh && ll >= rl);
  if (!(s.frames >= g.warm && s.sig >= g.min_p && ratio)) {
    s.state = kWait;
    return;
  }
  if (s.state == kWait) {
    if (lev) s.state = kIdle;
  } else if (s.state == kIdle) {
    if (!lev) {
      s.state = kChar;
      s.t = par.tb >> 1;
      s.bit = -1;
      s.code = 0;
      s.start = k;
    }
  } else {
    s.t -= 256;
    if (!samp) return;
    s.t += par.tb;
    if (s.bit < 0) {
      if (lev) {
        s.false_starts = sat_inc(s.false_starts);
        s.state = kIdle;
      } else {
        s.bit = 0;
      }
    } else if (s.bit < par.nbits) {
      s.code |= lev << s.bit;
      s.bit++;
    } else if (lev) {
      file_event(g, s, 0, ev, nev);
      s.state = kIdle;
    } else {
      file_event(g, s, 1, ev, nev);
      s.ferr = sat_inc(s.ferr);
      s.state = kWait;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_rtty(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ int A[kWaves][4][kRow];               // reduced sums: [0, kHist) the frames before the piece, then the piece's
  __shared__ unsigned long long Pb[kWaves][2][64];
  __shared__ long long carry[kWaves][4];
  __shared__ int lastsum[kWaves][4];
  RttyGeom const &g = c.g;
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * kWaves + wave;
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  kq::tonecorr::load_packed_table(CS, c.table, tid, kThreads);
  RttyPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const B = g.grid.B, L = c.L, F = 64 / L, f = lane / L, p = lane & (L - 1);
  int const W = live ? min(max(par.W, 1), kHist + 1) : 1;  // (the host keeps it in 8..32)
  unsigned const inc[2] = {par.inc_m, par.inc_s};
  // carried: lane 0 holds the record, the open frame's sums in it; the history goes to the front of A
  kq_rtty_status s{};
  unsigned nev = 0;
  kq_rtty_event *ev = c.ev + (size_t)slot * g.max_events;
  if (live && lane == 0) {
    s = c.state[slot];
    nev = c.nev[slot];
  }
  if (lane < kHist)
    for (int t = 0; t < 4; t++) A[wave][t][lane] = live ? c.hist[slot].v[t][lane] : 0;
  long long cy[4] = {s.acc_im, s.acc_qm, s.acc_is, s.acc_qs};
  int64_t n = c.n0, k0 = c.n0 / B;
  while (n < c.n1) {  // one piece: the frames k0 .. k0 + F - 1, from n to their end or the call's; x counts from k0 B
    int64_t const pe = (k0 + F) * (int64_t)B, e = pe < c.n1 ? pe : c.n1;
    int const x0 = (int)(n - k0 * B), x1 = x0 + (int)(e - n);  // x1 <= F B
    long long sm[4];  // (its first barrier: the piece before is done with q, A, Pb, carry and lastsum, and A is loaded)
    kq::tonecorr::correlate_piece<2>(g.grid, c.in, row, live, lane, L, c.n0, n, k0, x0, x1, qs[wave], CS, inc, sm, cy);
    int const done = (int)__umulhi((unsigned)x1, g.grid.magic);  // frames of the piece that are complete
    if (p == 0 && f * B < x1) {
      if (f < done) {
        for (int t = 0; t < 4; t++) A[wave][t][kHist + f] = (int)(sm[t] >> 12);
      } else {  // the call ends inside frame f
        for (int t = 0; t < 4; t++) carry[wave][t] = sm[t];
      }
    }
    __syncthreads();
    int keep[4] = {0, 0, 0, 0};
    if (lane < done) {  // the window that ends at frame `lane` of the piece: W entries, the last at kHist + lane
      int w[4] = {0, 0, 0, 0};
      for (int i = 0; i < W; i++)
        for (int t = 0; t < 4; t++) w[t] += A[wave][t][kHist + lane - i];
      Pb[wave][0][lane] = (unsigned long long)((long long)w[0] * w[0]) + (unsigned long long)((long long)w[1] * w[1]);
      Pb[wave][1][lane] = (unsigned long long)((long long)w[2] * w[2]) + (unsigned long long)((long long)w[3] * w[3]);
      if (lane == done - 1)
        for (int t = 0; t < 4; t++) lastsum[wave][t] = w[t];
    }
    if (lane < kHist)  // what the next piece finds in front: the last kHist frames
      for (int t = 0; t < 4; t++) keep[t] = A[wave][t][done + lane];
    __syncthreads();
    if (lane < kHist)
      for (int t = 0; t < 4; t++) A[wave][t][lane] = keep[t];
    if (live && lane == 0) {
      for (int i = 0; i < done; i++) step(g, par, s, Pb[wave][0][i], Pb[wave][1][i], (unsigned long long)(k0 + i), ev, nev);
      if (done) {
        s.sum_im = lastsum[wave][0];
        s.sum_qm = lastsum[wave][1];
        s.sum_is = lastsum[wave][2];
        s.sum_qs = lastsum[wave][3];
      }
      if (done * B < x1)
        for (int t = 0; t < 4; t++) cy[t] = carry[wave][t];
    }
    n = e;
    k0 += F;
  }
  __syncthreads();
  if (live && lane < kHist)
    for (int t = 0; t < 4; t++) c.hist[slot].v[t][lane] = A[wave][t][lane];
  if (live && lane == 0) {
    s.acc_im = cy[0];
    s.acc_qm = cy[1];
    s.acc_is = cy[2];
    s.acc_qs = cy[3];
    c.state[slot] = s;
    c.nev[slot] = nev;
    if (c.st) c.st[(size_t)slot * c.sstride] = s;
  }
}

}  // namespace

struct kq_rtty_bank : kq::HostSide {
  static constexpr bool kDeferred = true;
  kq_rtty_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  RttyGeom g{};
  int Lmin = 1;                  // the least lanes to a frame whose piece fits kTile
  uint64_t n_cur = 0;
  kq::DeferredSlots<RttyPar> def;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<RttyPar> slots;
    short *table = nullptr;
    kq_rtty_status *state = nullptr;
    RttyHist *hist = nullptr;
    kq::EventArena<kq_rtty_event> arena;
    kq_rtty_status *st = nullptr;        // host-memory calls
  } d;

  int to_device();
};

namespace {

int make_device(kq_rtty_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots;
  if (d.slots.alloc(*b, S) || kq::tonecorr::alloc_table(*b, &d.table) || b->alloc(&d.state, S, true) ||
      b->alloc(&d.hist, S, true) || d.arena.alloc(*b, S, b->cfg.max_events))
    return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // namespace

// kq::DeferredSlots::flush; the record and the history of a slot that is set start cold (all zero: the header's state at
// the set) and its arena empty
int kq_rtty_bank::to_device() {
  return def.flush(this, make_device, [this](size_t s0, size_t n) {
    KQ_TRY(hipMemsetAsync(d.state + s0, 0, n * sizeof(kq_rtty_status), stream));
    KQ_TRY(hipMemsetAsync(d.hist + s0, 0, n * sizeof(RttyHist), stream));
    return d.arena.clear(*this, s0, n);
  });
}

extern "C" {

kq_rtty_bank *kq_rtty_create(const kq_rtty_config *cfg) {
  const char *fn = "kq_rtty_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!kq::samprate_ok(fn, cfg->samprate) || !kq::field_in_range(fn, "block_len", cfg->block_len, 8, 256) ||
      !kq::field_in_range(fn, "warm", cfg->warm, 0, 65535) || !kq::field_in_range(fn, "snr", cfg->snr, 16, 4095) ||
      !kq::min_p_ok(fn, cfg->min_p) || !kq::input_scale_ok(fn, cfg->input_scale) ||
      !kq::field_in_range(fn, "max_slots", cfg->max_slots, 1, kMaxSlots) ||
      !kq::field_in_range(fn, "max_events", cfg->max_events, 1, 4096) || !kq::max_samples_ok(fn, cfg->max_samples))
    return nullptr;
  (void)kq::tonecorr::cos_table();  // the table exists from here on
  kq_rtty_bank *b = new kq_rtty_bank;
  b->cfg = *cfg;
  b->def.init(cfg->max_slots);
  RttyGeom &g = b->g;
  g.grid = kq::tonecorr::frame_grid(cfg->block_len);
  g.warm = cfg->warm;
  g.snr = cfg->snr;
  g.min_p = cfg->min_p;
  g.max_events = (int)cfg->max_events;
  b->Lmin = kq::tonecorr::least_lanes(g.grid, kTile);  // 8 at the most: Bs <= 258
  return b;
}

int kq_rtty_destroy(kq_rtty_bank *b) { return kq::destroy_bank(b, "kq_rtty_destroy"); }

int kq_rtty_set(kq_rtty_bank *b, unsigned slot, const kq_rtty_params *p) {
  const char *fn = "kq_rtty_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  double const Fs = b->cfg.samprate, fm = p->mark, fs = p->space, baud = p->baud;
  if (!(fm > 0) || !(fm < 0.5 * Fs)) {
    kq_internal_set_error("%s: mark %g must be above 0 and below samprate / 2", fn, fm);
    return -1;
  }
  if (!(fs > 0) || !(fs < 0.5 * Fs)) {
    kq_internal_set_error("%s: space %g must be above 0 and below samprate / 2", fn, fs);
    return -1;
  }
  if (p->mark == p->space) {
    kq_internal_set_error("%s: mark and space are both %g", fn, fm);
    return -1;
  }
  if (!kq::field_in_range(fn, "nbits", p->nbits, 5, 8)) return -1;
  if (!(baud > 0) || !std::isfinite(baud)) {
    kq_internal_set_error("%s: baud %g must be positive and finite", fn, baud);
    return -1;
  }
  double const tb = std::rint(256.0 * Fs / ((double)b->cfg.block_len * baud));
  if (!(tb >= 2048.0) || !(tb <= 8192.0)) {
    kq_internal_set_error("%s: baud %g makes tb %.10g, a bit of %g frames of %u samples, outside 2048..8192 (8 to 32 frames)", fn,
                          baud, tb, tb / 256.0, b->cfg.block_len);
    return -1;
  }
  RttyPar np{};
  np.active = 1;
  np.source = p->source;
  np.inc_m = (unsigned)std::llrint(fm * 4294967296.0 / Fs);
  np.inc_s = (unsigned)std::llrint(fs * 4294967296.0 / Fs);
  np.tb = (int)tb;
  np.W = (np.tb + 128) >> 8;
  np.nbits = (int)p->nbits;
  b->def.set(slot, np);
  return 0;
}

int kq_rtty_remove(kq_rtty_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_rtty_remove"); }

int kq_rtty_process(kq_rtty_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_rtty_status *status, size_t status_stride) {
  const char *fn = "kq_rtty_process";
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
  a.hist = d.hist;
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
  hipLaunchKernelGGL(k_rtty, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_rtty_pull_counts(kq_rtty_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_rtty_pull_counts", counts); }

int kq_rtty_pull_event(kq_rtty_bank *b, unsigned slot, unsigned index, kq_rtty_event *event) {
  return kq::pull_event(b, "kq_rtty_pull_event", slot, index, event);
}

int kq_rtty_clear_events(kq_rtty_bank *b) { return kq::clear_arena(b, "kq_rtty_clear_events"); }

int kq_rtty_get_table(const kq_rtty_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_rtty_get_table", dst, cap);
}

int kq_rtty_get_slot(kq_rtty_bank *b, unsigned slot, kq_rtty_slot *out) {
  if (!b) {
    kq_internal_set_error("kq_rtty_get_slot: null bank");
    return -1;
  }
  if (!out) {
    kq_internal_set_error("kq_rtty_get_slot: null out");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("kq_rtty_get_slot: slot %u holds no decoder", slot);
    return -1;
  }
  RttyPar const &w = b->def.want[slot];
  out->inc_m = w.inc_m;
  out->inc_s = w.inc_s;
  out->tb = (uint32_t)w.tb;
  out->W = (uint32_t)w.W;
  return 0;
}

int kq_rtty_sync(kq_rtty_bank *b) { return kq::sync_bank(b, "kq_rtty_sync"); }

int kq_rtty_reset(kq_rtty_bank *b) { return kq::deferred_reset(b, "kq_rtty_reset"); }

}  // extern "C"
