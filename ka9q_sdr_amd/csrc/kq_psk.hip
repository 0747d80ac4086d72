// kq_psk.hip -- PSK31 / PSK63 / PSK125 decoder bank: the audio of SSB channels -> Varicode characters, as events (code,
// flags, end, sig, rotation) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_psk_*): quantise as kq_cw_*, correlate every frame of B samples against one tone from
// the 1024-entry cosine table with a phase that is a function of the sample index alone, slide a window one symbol long
// (W frames) over the frames' reduced sums, and step the symbol clock once per completed frame; at every third point of
// the clock a symbol is read: the differential product against the symbol before, the decision against the rotation
// estimate, the levels and the Varicode shift register.  All exact integers after the quantiser.  State on the device,
// per slot: one kq_psk_status record, the reduced sums of the last 31 frames, and the arena of events; per bank the
// table.
//
// k_psk   k_rtty's mapping: one wave per slot, four slots to a workgroup.  The call's samples go through LDS once, a piece
//         of 64 / L frames at a time (kq::tonecorr::correlate_piece<1>).  The frame leaders write the two reduced sums to
//         LDS behind the 31 carried frames of history (W <= 32), lane f then sums its own W entries and squares -- exact,
//         so no scan order matters -- and lane 0 walks the piece's (SI, SQ, P) in order through the clock: most frames
//         cost it a subtraction and a compare, and it reads LDS at the points only.  The baud rate and W differ from slot
//         to slot; B and the frame grid do not, so every wave of a workgroup has the same pieces and the barriers are
//         uniform.  The carried record and the history are read once and written once per call.  No atomics, no scratch.
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

struct PskGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr;
  unsigned long long min_p;
  int max_events;
};

struct PskPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc;
  int tb, W;
};

struct PskHist {
  int v[2][kHist];               // a, b; [kHist - 1] is the last completed frame
};

struct CallArgs {
  PskGeom g;
  const PskPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;            // [1024]
  kq_psk_status *state;          // [S]
  PskHist *hist;                 // [S]
  kq_psk_event *ev;              // [S][max_events]
  unsigned *nev;                 // [S]
  int nlist;
  int L;                         // lanes to a frame, a power of two <= 64
  int64_t n0, n1;                // the call's samples
  kq::PcmIn in;
  // output
  kq_psk_status *st;
  size_t sstride;
};

__device__ __forceinline__ unsigned sat_inc(unsigned v) { return v == 0xFFFFFFFFu ? v : v + 1; }

__device__ __forceinline__ long long mag(long long v) { return v < 0 ? -v : v; }

// the header's norm: both shifted down until the larger magnitude is below 2^24
__device__ __forceinline__ void norm24(long long x, long long y, long long &nx, long long &ny) {
  unsigned long long const m = (unsigned long long)(mag(x) > mag(y) ? mag(x) : mag(y));
  int const len = m ? 64 - __clzll((long long)m) : 0, s = len > 24 ? len - 24 : 0;
  nx = x >> s;
  ny = y >> s;
}

// the header's steps 1 to 8: the late point of a symbol at frame k, with the late power pl
__device__ __forceinline__ void symbol(PskGeom const &g, PskPar const &par, kq_psk_status &s, unsigned long long pl,
                                       unsigned long long k, kq_psk_event *ev, unsigned &nev) {
  // 1 timing (every value is below 2^61: the differences fit)
  s.ee = (unsigned long long)((long long)s.ee + (((long long)s.pe - (long long)s.ee) >> 3));
  s.el = (unsigned long long)((long long)s.el + (((long long)pl - (long long)s.el) >> 3));
  unsigned long long const m = s.ee > s.el ? s.ee : s.el;
  int adj = 0;
  if (s.ee > s.el && s.ee - s.el > (m >> 3)) adj = -(par.tb >> 5);
  else if (s.el > s.ee && s.el - s.ee > (m >> 3)) adj = par.tb >> 5;
  s.t += par.tb - 2 * (par.tb >> 2) + adj;
  // 2 product
  long long const cr = s.cr, ci = s.ci, pr = s.pr, pi = s.pi;
  long long const Dr = cr * pr + ci * pi, Di = ci * pr - cr * pi;
  s.pr = s.cr;
  s.pi = s.ci;
  // 3 normalise
  long long dr, di, rr = 1, ri = 0;
  norm24(Dr, Di, dr, di);
  if (s.rot_r | s.rot_i) norm24(s.rot_r, s.rot_i, rr, ri);
  // 4 decision
  long long const Re = dr * rr + di * ri, Im = di * rr - dr * ri;
  bool const bit = Re >= 0;
  // 5 rotation
  s.rot_r += ((bit ? Dr : -Dr) - s.rot_r) >> 4;
  s.rot_i += ((bit ? Di : -Di) - s.rot_i) >> 4;
  if (2 * s.rot_r < mag(s.rot_i)) s.rot_r = mag(s.rot_i) >> 1;
  // 6 levels
  s.qre = (unsigned long long)((long long)s.qre + ((mag(Re) - (long long)s.qre) >> 4));
  s.qim = (unsigned long long)((long long)s.qim + ((mag(Im) - (long long)s.qim) >> 4));
  s.sig = (unsigned long long)((long long)s.sig + (((long long)s.pc - (long long)s.sig) >> 4));
  // 7 validity
  if (!(s.frames >= g.warm && s.sig >= g.min_p && 16 * s.qre >= (unsigned long long)g.snr * s.qim)) {
    s.shreg = 0;
    s.over = 0;
    return;
  }
  // 8 Varicode
  if (s.shreg & 0x2000u) s.over = 1;
  s.shreg = (s.shreg << 1 | (bit ? 1u : 0u)) & 0x3FFFu;
  if ((s.shreg & 3u) == 0) {
    unsigned const code = s.shreg >> 2;
    if (code) {
      s.events = sat_inc(s.events);
      if (nev >= (unsigned)g.max_events) {
        s.dropped = sat_inc(s.dropped);
      } else {
        kq_psk_event r;
        r.code = code;
        r.flags = code > 1023 ? 1u : s.over;
        r.end_sample = (k + 1) * (unsigned long long)g.grid.B;
        r.sig = s.sig;
        r.rot_r = (int)rr;
        r.rot_i = (int)ri;
        ev[nev++] = r;
      }
    }
    s.shreg = 0;
    s.over = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_psk(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ int A[kWaves][2][kRow];               // reduced sums: [0, kHist) the frames before the piece, then the piece's
  __shared__ unsigned long long Pb[kWaves][64];    // the window's power at every frame of the piece
  __shared__ int Sb[kWaves][2][64];                // and its sums
  __shared__ long long carry[kWaves][2];
  PskGeom const &g = c.g;
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * kWaves + wave;
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  kq::tonecorr::load_packed_table(CS, c.table, tid, kThreads);
  PskPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const B = g.grid.B, L = c.L, F = 64 / L, f = lane / L, p = lane & (L - 1);
  int const W = live ? min(max(par.W, 1), kHist + 1) : 1;  // (the host keeps it in 8..32)
  int const q = par.tb >> 2;
  unsigned const inc[1] = {par.inc};
  // carried: lane 0 holds the record, the open frame's sums in it; the history goes to the front of A
  kq_psk_status s{};
  unsigned nev = 0;
  kq_psk_event *ev = c.ev + (size_t)slot * g.max_events;
  if (live && lane == 0) {
    s = c.state[slot];
    nev = c.nev[slot];
  }
  if (lane < kHist)
    for (int t = 0; t < 2; t++) A[wave][t][lane] = live ? c.hist[slot].v[t][lane] : 0;
  long long cy[2] = {s.acc_i, s.acc_q};
  int64_t n = c.n0, k0 = c.n0 / B;
  while (n < c.n1) {  // one piece: the frames k0 .. k0 + F - 1, from n to their end or the call's; x counts from k0 B
    int64_t const pe = (k0 + F) * (int64_t)B, e = pe < c.n1 ? pe : c.n1;
    int const x0 = (int)(n - k0 * B), x1 = x0 + (int)(e - n);  // x1 <= F B
    long long sm[2];  // (its first barrier: the piece before is done with q, A, Pb, Sb and carry, and A is loaded)
    kq::tonecorr::correlate_piece<1>(g.grid, c.in, row, live, lane, L, c.n0, n, k0, x0, x1, qs[wave], CS, inc, sm, cy);
    int const done = (int)__umulhi((unsigned)x1, g.grid.magic);  // frames of the piece that are complete
    if (p == 0 && f * B < x1) {
      if (f < done) {
        for (int t = 0; t < 2; t++) A[wave][t][kHist + f] = (int)(sm[t] >> 13);
      } else {  // the call ends inside frame f
        for (int t = 0; t < 2; t++) carry[wave][t] = sm[t];
      }
    }
    __syncthreads();
    int keep[2] = {0, 0};
    if (lane < done) {  // the window that ends at frame `lane` of the piece: W entries, the last at kHist + lane
      int w[2] = {0, 0};
      for (int i = 0; i < W; i++)
        for (int t = 0; t < 2; t++) w[t] += A[wave][t][kHist + lane - i];
      Pb[wave][lane] = (unsigned long long)((long long)w[0] * w[0]) + (unsigned long long)((long long)w[1] * w[1]);
      Sb[wave][0][lane] = w[0];
      Sb[wave][1][lane] = w[1];
    }
    if (lane < kHist)  // what the next piece finds in front: the last kHist frames
      for (int t = 0; t < 2; t++) keep[t] = A[wave][t][done + lane];
    __syncthreads();
    if (lane < kHist)
      for (int t = 0; t < 2; t++) A[wave][t][lane] = keep[t];
    if (live && lane == 0) {
      for (int i = 0; i < done; i++) {  // the header's step, frame k0 + i
        s.frames = sat_inc(s.frames);
        s.t -= 256;
        if (s.t >= 128) continue;
        unsigned long long const P = Pb[wave][i];
        if (s.ph == 0) {
          s.pe = P;
          s.t += q;
          s.ph = 1;
        } else if (s.ph == 1) {
          s.cr = Sb[wave][0][i];
          s.ci = Sb[wave][1][i];
          s.pc = P;
          s.t += q;
          s.ph = 2;
        } else {
          s.ph = 0;
          symbol(g, par, s, P, (unsigned long long)(k0 + i), ev, nev);
        }
      }
      if (done) {
        s.sum_i = Sb[wave][0][done - 1];
        s.sum_q = Sb[wave][1][done - 1];
      }
      if (done * B < x1)
        for (int t = 0; t < 2; t++) cy[t] = carry[wave][t];
    }
    n = e;
    k0 += F;
  }
  __syncthreads();
  if (live && lane < kHist)
    for (int t = 0; t < 2; t++) c.hist[slot].v[t][lane] = A[wave][t][lane];
  if (live && lane == 0) {
    s.acc_i = cy[0];
    s.acc_q = cy[1];
    c.state[slot] = s;
    c.nev[slot] = nev;
    if (c.st) c.st[(size_t)slot * c.sstride] = s;
  }
}

}  // namespace

struct kq_psk_bank : kq::HostSide {
  static constexpr bool kDeferred = true;
  kq_psk_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  PskGeom g{};
  int Lmin = 1;                  // the least lanes to a frame whose piece fits kTile
  uint64_t n_cur = 0;
  kq::DeferredSlots<PskPar> def;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<PskPar> slots;
    short *table = nullptr;
    kq_psk_status *state = nullptr;
    PskHist *hist = nullptr;
    kq::EventArena<kq_psk_event> arena;
    kq_psk_status *st = nullptr;         // host-memory calls
  } d;

  int to_device();
};

namespace {

int make_device(kq_psk_bank *b) {
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
int kq_psk_bank::to_device() {
  return def.flush(this, make_device, [this](size_t s0, size_t n) {
    KQ_TRY(hipMemsetAsync(d.state + s0, 0, n * sizeof(kq_psk_status), stream));
    KQ_TRY(hipMemsetAsync(d.hist + s0, 0, n * sizeof(PskHist), stream));
    return d.arena.clear(*this, s0, n);
  });
}

extern "C" {

kq_psk_bank *kq_psk_create(const kq_psk_config *cfg) {
  const char *fn = "kq_psk_create";
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
  kq_psk_bank *b = new kq_psk_bank;
  b->cfg = *cfg;
  b->def.init(cfg->max_slots);
  PskGeom &g = b->g;
  g.grid = kq::tonecorr::frame_grid(cfg->block_len);
  g.warm = cfg->warm;
  g.snr = cfg->snr;
  g.min_p = cfg->min_p;
  g.max_events = (int)cfg->max_events;
  b->Lmin = kq::tonecorr::least_lanes(g.grid, kTile);  // 8 at the most: Bs <= 258
  return b;
}

int kq_psk_destroy(kq_psk_bank *b) { return kq::destroy_bank(b, "kq_psk_destroy"); }

int kq_psk_set(kq_psk_bank *b, unsigned slot, const kq_psk_params *p) {
  const char *fn = "kq_psk_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  double const Fs = b->cfg.samprate, pitch = p->pitch, baud = p->baud;
  if (!(pitch > 0) || !(pitch < 0.5 * Fs)) {
    kq_internal_set_error("%s: pitch %g must be above 0 and below samprate / 2", fn, pitch);
    return -1;
  }
  if (!(baud > 0) || !std::isfinite(baud)) {
    kq_internal_set_error("%s: baud %g must be positive and finite", fn, baud);
    return -1;
  }
  double const tb = std::rint(256.0 * Fs / ((double)b->cfg.block_len * baud));
  if (!(tb >= 2048.0) || !(tb <= 8192.0)) {
    kq_internal_set_error("%s: baud %g makes tb %.10g, a symbol of %g frames of %u samples, outside 2048..8192 (8 to 32 frames)",
                          fn, baud, tb, tb / 256.0, b->cfg.block_len);
    return -1;
  }
  PskPar np{};
  np.active = 1;
  np.source = p->source;
  np.inc = (unsigned)std::llrint(pitch * 4294967296.0 / Fs);
  np.tb = (int)tb;
  np.W = (np.tb + 128) >> 8;
  b->def.set(slot, np);
  return 0;
}

int kq_psk_remove(kq_psk_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_psk_remove"); }

int kq_psk_process(kq_psk_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_psk_status *status, size_t status_stride) {
  const char *fn = "kq_psk_process";
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
  hipLaunchKernelGGL(k_psk, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_psk_pull_counts(kq_psk_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_psk_pull_counts", counts); }

int kq_psk_pull_event(kq_psk_bank *b, unsigned slot, unsigned index, kq_psk_event *event) {
  return kq::pull_event(b, "kq_psk_pull_event", slot, index, event);
}

int kq_psk_clear_events(kq_psk_bank *b) { return kq::clear_arena(b, "kq_psk_clear_events"); }

int kq_psk_get_table(const kq_psk_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_psk_get_table", dst, cap);
}

int kq_psk_get_slot(kq_psk_bank *b, unsigned slot, kq_psk_slot *out) {
  if (!b) {
    kq_internal_set_error("kq_psk_get_slot: null bank");
    return -1;
  }
  if (!out) {
    kq_internal_set_error("kq_psk_get_slot: null out");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("kq_psk_get_slot: slot %u holds no decoder", slot);
    return -1;
  }
  PskPar const &w = b->def.want[slot];
  out->inc = w.inc;
  out->tb = (uint32_t)w.tb;
  out->W = (uint32_t)w.W;
  out->reserved = 0;
  return 0;
}

int kq_psk_sync(kq_psk_bank *b) { return kq::sync_bank(b, "kq_psk_sync"); }

int kq_psk_reset(kq_psk_bank *b) { return kq::deferred_reset(b, "kq_psk_reset"); }

}  // extern "C"
