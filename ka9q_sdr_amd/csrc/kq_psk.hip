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
// k_psk   a frame-grid kernel with a window and a symbol clock (kq_tonecorr.hpp describes the mapping): one tone, two
//         series.  Lane f sums its own W entries per series and squares, and lane 0 walks the piece's (SI, SQ, P) in order
//         through the clock: it reads LDS at the points only.
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
using tc::mag;
using tc::sat_inc;
constexpr unsigned kMaxSlots = 16384;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50; with the rest
                                                // the workgroup stays under 40 KiB, four workgroups to a CU
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

struct PskKind {
  using Config = kq_psk_config;
  using Geom = PskGeom;
  using Par = PskPar;
  using Status = kq_psk_status;
  using Event = kq_psk_event;
  using Hist = tc::FrameHist<2>;  // a, b
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
};
using CallArgs = tc::GridBank<PskKind>::Args;

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
  // 1 timing
  tc::clock_adjust(s, par.tb, pl);
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
  tc::smooth(s.qre, (uint64_t)mag(Re), 4);
  tc::smooth(s.qim, (uint64_t)mag(Im), 4);
  tc::smooth(s.sig, s.pc, 4);
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
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane, W = tc::window_frames(w.live, w.par.W);
  int const q = w.par.tb >> 2;
  unsigned const inc[1] = {w.par.inc};
  kq_psk_status s{};
  unsigned nev = 0;
  kq_psk_event *ev = tc::load_record(c, w, s, nev);
  if (lane < kHist)  // (tc::load_hist and tc::store_hist, the same lines, measured 0.6 % slower at 4096-sample calls here)
    for (int t = 0; t < 2; t++) A[wave][t][lane] = w.live ? c.hist[w.slot].v[t][lane] : 0;
  long long cy[2] = {s.acc_i, s.acc_q};
  for (tc::Piece pc(c.n0, w.B); pc.n < c.n1; pc.next(w.F)) {
    pc.span(c.n1, w.B, w.F);
    long long sm[2];  // (its first barrier: the piece before is done with q, A, Pb, Sb and carry, and A is loaded)
    tc::correlate_piece<1>(c, w, pc, qs[wave], CS, inc, sm, cy);
    int const done = pc.done(g.grid);
    tc::file_sums(A[wave], carry[wave], w, pc, done, sm, 13);
    __syncthreads();
    int keep[2] = {0, 0};
    if (lane < done) {
      int wi = 0, wq = 0;  // the window that ends at frame `lane`: W entries, the last at kHist + lane; both series side by
      for (int i = 0; i < W; i++) {  // side, as k_rtty's (one after the other, tc::window_sum, was no faster)
        wi += A[wave][0][kHist + lane - i];
        wq += A[wave][1][kHist + lane - i];
      }
      Pb[wave][lane] = (unsigned long long)((long long)wi * wi) + (unsigned long long)((long long)wq * wq);
      Sb[wave][0][lane] = wi;
      Sb[wave][1][lane] = wq;
    }
    tc::keep_hist(A[wave], lane, done, keep);
    __syncthreads();
    tc::put_hist(A[wave], lane, keep);
    if (w.live && lane == 0) {
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
          symbol(g, w.par, s, P, (unsigned long long)(pc.k0 + i), ev, nev);
        }
      }
      if (done) {
        s.sum_i = Sb[wave][0][done - 1];
        s.sum_q = Sb[wave][1][done - 1];
      }
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  __syncthreads();
  if (w.live && lane < kHist)
    for (int t = 0; t < 2; t++) c.hist[w.slot].v[t][lane] = A[wave][t][lane];
  s.acc_i = cy[0];
  s.acc_q = cy[1];
  tc::store_record(c, w, s, nev);
}

}  // namespace

struct kq_psk_bank : tc::GridBank<PskKind> {};

extern "C" {

kq_psk_bank *kq_psk_create(const kq_psk_config *cfg) {
  const char *fn = "kq_psk_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !tc::config_tail_ok(fn, cfg, kMaxSlots)) return nullptr;
  return tc::finish_create<kq_psk_bank>(cfg, kTile);  // Lmin 8 at the most: Bs <= 258
}

int kq_psk_destroy(kq_psk_bank *b) { return kq::destroy_bank(b, "kq_psk_destroy"); }

int kq_psk_set(kq_psk_bank *b, unsigned slot, const kq_psk_params *p) {
  const char *fn = "kq_psk_set";
  std::unique_lock<std::mutex> lk;
  if (!tc::open_set(b, fn, slot, p, kMaxSlots, lk)) return -1;
  double const Fs = b->cfg.samprate, pitch = p->pitch;
  PskPar np{};
  if (!tc::tone_ok(fn, Fs, pitch, "pitch %g", pitch) || !tc::symbol_period(fn, Fs, b->cfg.block_len, p->baud, "symbol", &np.tb, &np.W))
    return -1;
  np.active = 1;
  np.source = p->source;
  np.inc = (unsigned)std::llrint(pitch * 4294967296.0 / Fs);
  b->def.set(slot, np);
  return 0;
}

int kq_psk_remove(kq_psk_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_psk_remove"); }

int kq_psk_process(kq_psk_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_psk_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_psk_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL(k_psk, dim3(blocks), dim3(kThreads), 0, b->stream, a);
                               });
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
  std::unique_lock<std::mutex> lk;
  const PskPar *w = tc::wanted(b, "kq_psk_get_slot", slot, out, "out", lk);
  if (!w) return -1;
  out->inc = w->inc;
  out->tb = (uint32_t)w->tb;
  out->W = (uint32_t)w->W;
  out->reserved = 0;
  return 0;
}

int kq_psk_sync(kq_psk_bank *b) { return kq::sync_bank(b, "kq_psk_sync"); }

int kq_psk_reset(kq_psk_bank *b) { return kq::deferred_reset(b, "kq_psk_reset"); }

}  // extern "C"
