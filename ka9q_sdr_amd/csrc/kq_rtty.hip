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
// k_rtty  a frame-grid kernel with a window (kq_tonecorr.hpp describes the mapping): two tones, four series.  Lane f sums
//         its own W entries per series and squares, and lane 0 walks the piece's (Pm, Ps) pairs in order through the
//         levels and the framer.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <mutex>

#include "ka9q_hip.h"
#include "kq_tonecorr.hpp"

namespace tc = kq::tonecorr;

namespace {

using tc::kHist;
using tc::kTable;
using tc::sat_inc;
constexpr unsigned kMaxSlots = 16384;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50; with the rest
                                                // the workgroup stays under 40 KiB, four workgroups to a CU
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

struct RttyKind {
  using Config = kq_rtty_config;
  using Geom = RttyGeom;
  using Par = RttyPar;
  using Status = kq_rtty_status;
  using Event = kq_rtty_event;
  using Hist = tc::FrameHist<4>;  // a, b of mark, a, b of space
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
};
using CallArgs = tc::GridBank<RttyKind>::Args;

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
  if (s.state != kChar || samp) {
    int const sh = samp ? 4 : 6;
    tc::smooth(s.sig, hi, sh);
    tc::smooth(s.nse, lo, sh);
  }
  bool const ratio = tc::gate16(s.sig, s.nse, g.snr);
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
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane, W = tc::window_frames(w.live, w.par.W);
  unsigned const inc[2] = {w.par.inc_m, w.par.inc_s};
  kq_rtty_status s{};
  unsigned nev = 0;
  kq_rtty_event *ev = tc::load_record(c, w, s, nev);
  tc::load_hist(A[wave], c.hist, w);
  long long cy[4] = {s.acc_im, s.acc_qm, s.acc_is, s.acc_qs};
  for (tc::Piece pc(c.n0, w.B); pc.n < c.n1; pc.next(w.F)) {
    pc.span(c.n1, w.B, w.F);
    long long sm[4];  // (its first barrier: the piece before is done with q, A, Pb, carry and lastsum, and A is loaded)
    tc::correlate_piece<2>(c, w, pc, qs[wave], CS, inc, sm, cy);
    int const done = pc.done(g.grid);
    tc::file_sums(A[wave], carry[wave], w, pc, done, sm, 12);
    __syncthreads();
    int keep[4] = {0, 0, 0, 0};
    if (lane < done) {
      int v[4] = {0, 0, 0, 0};  // the window that ends at frame `lane`: W entries, the last at kHist + lane; the four series
      for (int i = 0; i < W; i++)  // side by side (a series after a series, tc::window_sum: 18 more VGPRs, 1 % slower)
        for (int t = 0; t < 4; t++) v[t] += A[wave][t][kHist + lane - i];
      Pb[wave][0][lane] = (unsigned long long)((long long)v[0] * v[0]) + (unsigned long long)((long long)v[1] * v[1]);
      Pb[wave][1][lane] = (unsigned long long)((long long)v[2] * v[2]) + (unsigned long long)((long long)v[3] * v[3]);
      if (lane == done - 1)
        for (int t = 0; t < 4; t++) lastsum[wave][t] = v[t];
    }
    tc::keep_hist(A[wave], lane, done, keep);
    __syncthreads();
    tc::put_hist(A[wave], lane, keep);
    if (w.live && lane == 0) {
      for (int i = 0; i < done; i++) step(g, w.par, s, Pb[wave][0][i], Pb[wave][1][i], (unsigned long long)(pc.k0 + i), ev, nev);
      if (done) {
        s.sum_im = lastsum[wave][0];
        s.sum_qm = lastsum[wave][1];
        s.sum_is = lastsum[wave][2];
        s.sum_qs = lastsum[wave][3];
      }
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  __syncthreads();
  tc::store_hist(A[wave], c.hist, w);
  s.acc_im = cy[0];
  s.acc_qm = cy[1];
  s.acc_is = cy[2];
  s.acc_qs = cy[3];
  tc::store_record(c, w, s, nev);
}

}  // namespace

struct kq_rtty_bank : tc::GridBank<RttyKind> {};

extern "C" {

kq_rtty_bank *kq_rtty_create(const kq_rtty_config *cfg) {
  const char *fn = "kq_rtty_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !tc::config_tail_ok(fn, cfg, kMaxSlots)) return nullptr;
  return tc::finish_create<kq_rtty_bank>(cfg, kTile);  // Lmin 8 at the most: Bs <= 258
}

int kq_rtty_destroy(kq_rtty_bank *b) { return kq::destroy_bank(b, "kq_rtty_destroy"); }

int kq_rtty_set(kq_rtty_bank *b, unsigned slot, const kq_rtty_params *p) {
  const char *fn = "kq_rtty_set";
  std::unique_lock<std::mutex> lk;
  if (!tc::open_set(b, fn, slot, p, kMaxSlots, lk)) return -1;
  double const Fs = b->cfg.samprate;
  RttyPar np{};
  if (!tc::tone_pair(fn, Fs, p->mark, p->space, &np.inc_m, &np.inc_s) || !kq::field_in_range(fn, "nbits", p->nbits, 5, 8) ||
      !tc::symbol_period(fn, Fs, b->cfg.block_len, p->baud, "bit", &np.tb, &np.W))
    return -1;
  np.active = 1;
  np.source = p->source;
  np.nbits = (int)p->nbits;
  b->def.set(slot, np);
  return 0;
}

int kq_rtty_remove(kq_rtty_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_rtty_remove"); }

int kq_rtty_process(kq_rtty_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_rtty_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_rtty_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL(k_rtty, dim3(blocks), dim3(kThreads), 0, b->stream, a);
                               });
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
  std::unique_lock<std::mutex> lk;
  const RttyPar *w = tc::wanted(b, "kq_rtty_get_slot", slot, out, "out", lk);
  if (!w) return -1;
  tc::get_pair_slot(*w, out);
  return 0;
}

int kq_rtty_sync(kq_rtty_bank *b) { return kq::sync_bank(b, "kq_rtty_sync"); }

int kq_rtty_reset(kq_rtty_bank *b) { return kq::deferred_reset(b, "kq_rtty_reset"); }

}  // extern "C"
