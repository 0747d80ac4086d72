// kq_same.hip -- EAS / SAME (Specific Area Message Encoding: 47 CFR 11.31, NWS Instruction 10-1712) decoder bank: the audio
// of broadcast and weather-radio channels -> one event per burst start, per byte of the header and per burst end (code,
// flags, index, errs, end, sig, nse) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_same_*): kq_dsc_*'s front half and bit clock to the letter -- quantise, correlate every
// frame of B samples against the mark and the space tone, slide a window one bit long over the frames' reduced sums, step
// the three-point clock once per completed frame -- and at every third point of the clock a bit is read: the levels, the
// gate, the 64-bit register, and -- at every bit while there is no sync -- the attempt on the preamble's end with ZCZC or
// NNNN behind it; in sync, at every eighth bit a byte, filed as it is, and the three ways a burst ends.  All exact integers
// after the quantiser.  State on the device, per slot: one kq_same_status record, the reduced sums of the last 31 frames,
// and the arena of events; per bank the table.  The signal format is written down from memory (the header says so).
//
// k_same    k_dsc's frame-grid kernel with another tracker above the bit.  The format is ASCII behind a fixed preamble, so
//           the device needs no table: two 48-bit patterns and a range test.  There is no open message: the whole record,
//           49 words, travels through lane 0 (tc::load_record, tc::store_record).  It is a word longer than k_navtex's,
//           which sat on the bound of 128 VGPRs, so what a bit seldom touches waits in LDS between the load and the store
//           and not in lane 0's registers: the five burst counters and sync_sample (tally, 32 bytes a wave) and the window
//           sums of the last completed frame (lastsum, which k_dsc's front half has anyway).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "ka9q_hip.h"
#include "kq_tonecorr.hpp"

namespace tc = kq::tonecorr;

namespace {

using tc::kHist;
using tc::kTable;
using tc::sat_inc;
using tc::smooth;
constexpr unsigned kMaxSlots = 16384;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 3200;                     // samples a wave keeps in LDS, as k_dsc: the workgroup stays under 40 KiB
constexpr int kRow = kHist + 64 + 1;            // a wave's reduced sums of one kind: the history and a piece's frames
constexpr unsigned kStart = 1, kBad = 2, kEnd = 4;
constexpr unsigned kComplete = 1, kLost = 2, kLength = 3;  // an END event's code
enum { kSyncs, kEoms, kCompleteN, kLostN, kTruncated, kSampleLo, kSampleHi, kTally };  // a wave's tally in LDS
// AB AB 'Z' 'C' 'Z' 'C' and AB AB 'N' 'N' 'N' 'N', the first byte sent highest, each byte bit-reversed (the first bit sent
// is a byte's bit 0, and the register takes the first bit sent highest)
constexpr unsigned long long kHeader = 0xD5D55AC25AC2ull, kEom = 0xD5D572727272ull, kMask48 = 0xFFFFFFFFFFFFull;

struct SameGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr, sync_errs, lose, max_len;
  unsigned long long min_p;
  int max_events;
};

struct SamePar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc_m, inc_s;
  int tb, W;
};

struct SameKind {
  using Config = kq_same_config;
  using Geom = SameGeom;
  using Par = SamePar;
  using Status = kq_same_status;
  using Event = kq_same_event;
  using Hist = tc::FrameHist<4>;  // a, b of mark, a, b of space
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
};
using CallArgs = tc::GridBank<SameKind>::Args;

__device__ __forceinline__ void file(SameGeom const &g, kq_same_status &s, unsigned code, unsigned flags, unsigned index,
                                     unsigned errs, unsigned long long k, kq_same_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_same_event &r = ev[nev++];
  r.code = code;
  r.flags = flags;
  r.index = index;
  r.errs = errs;
  r.end_sample = (k + 1) * (unsigned long long)g.grid.B;
  r.sig = s.sig;
  r.nse = s.nse;
}

// the header's steps 1 to 5: the late point of a bit at frame k, with the late power pl
__device__ __forceinline__ void bit_step(SameGeom const &g, SamePar const &par, kq_same_status &s, unsigned long long pl,
                                         unsigned long long k, kq_same_event *ev, unsigned &nev, unsigned *tally) {
  // 1 timing
  tc::clock_adjust(s, par.tb, pl);
  smooth(s.ec, s.hi, 3);
  unsigned long long const top = s.ee > s.el ? s.ee : s.el, low = s.ee > s.el ? s.el : s.ee;
  if (top - low <= (top >> 3) && s.ec + (top >> 3) < low) s.t += par.tb >> 5;  // (adj == 0) half a bit out: no slope there
  // 2 levels and gate
  smooth(s.sig, s.hi, 4);
  smooth(s.nse, s.lo, 4);
  bool const open = s.frames >= g.warm && s.sig >= g.min_p && tc::gate16(s.sig, s.nse, g.snr);
  // 3 register
  s.r = s.r << 1 | (unsigned long long)s.bit;
  // 4 sync
  if (!s.synced) {
    if (!open) return;
    unsigned const dh = (unsigned)__popcll((s.r ^ kHeader) & kMask48), de = (unsigned)__popcll((s.r ^ kEom) & kMask48);
    if (dh <= g.sync_errs || de <= g.sync_errs) {  // sync_sample
      unsigned long long const at = (k + 1) * (unsigned long long)g.grid.B;
      tally[kSampleLo] = (unsigned)at;
      tally[kSampleHi] = (unsigned)(at >> 32);
    }
    if (dh <= g.sync_errs) {
      s.synced = 1;
      s.bitpos = s.nbytes = s.bad_run = s.plus = s.dashes = 0;
      tally[kSyncs] = sat_inc(tally[kSyncs]);
      file(g, s, 'Z', kStart, 0, dh, k, ev, nev);
    } else if (de <= g.sync_errs) {
      tally[kEoms] = sat_inc(tally[kEoms]);
      file(g, s, 'N', kStart, 0, de, k, ev, nev);
    }
    return;
  }
  // 5 text
  s.bitpos += 1;
  if (s.bitpos < 8) return;
  s.bitpos = 0;
  unsigned const b = __brev((unsigned)s.r << 24) & 255u;
  if (b >= 0x20 && b <= 0x7E) {
    file(g, s, b, 0, s.nbytes, 0, k, ev, nev);
    s.bad_run = 0;
    if (b == '+') s.plus = 1;
    else if (b == '-' && s.plus) s.dashes += 1;
  } else {
    file(g, s, b, kBad, s.nbytes, 0, k, ev, nev);
    s.bad_run += 1;
  }
  s.nbytes += 1;
  unsigned why = 0;
  if (s.dashes == 3) {
    why = kComplete;
    tally[kCompleteN] = sat_inc(tally[kCompleteN]);
  } else if (s.bad_run == g.lose) {
    why = kLost;
    tally[kLostN] = sat_inc(tally[kLostN]);
  } else if (s.nbytes == g.max_len) {
    why = kLength;
    tally[kTruncated] = sat_inc(tally[kTruncated]);
  }
  if (!why) return;
  file(g, s, why, kEnd, s.nbytes, 0, k, ev, nev);
  s.synced = 0;
}

// (four waves to a SIMD asked for, as k_dsc: four workgroups to a CU need 128 VGPRs or fewer)
__global__ __launch_bounds__(kThreads, 4) void k_same(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ int A[kWaves][4][kRow];               // reduced sums: [0, kHist) the frames before the piece, then the piece's
  __shared__ unsigned long long Pb[kWaves][2][64];
  __shared__ long long carry[kWaves][4];
  __shared__ int lastsum[kWaves][4];
  __shared__ unsigned tally[kWaves][kTally];
  SameGeom const &g = c.g;
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane, W = tc::window_frames(w.live, w.par.W);
  unsigned const inc[2] = {w.par.inc_m, w.par.inc_s};
  int const q = w.par.tb >> 2;
  kq_same_status s{};
  unsigned nev = 0;
  kq_same_event *ev = tc::load_record(c, w, s, nev);
  tc::load_hist(A[wave], c.hist, w);
  long long cy[4] = {s.acc[0][0], s.acc[0][1], s.acc[1][0], s.acc[1][1]};
  // what waits in LDS (see the top): lastsum, which a piece without a completed frame leaves alone, and the tally.  Lane 0
  // alone touches the tally; lastsum's other writers stand behind the first barrier below
  if (w.live && lane == 0) {
    tally[wave][kSyncs] = s.syncs;
    tally[wave][kEoms] = s.eoms;
    tally[wave][kCompleteN] = s.complete;
    tally[wave][kLostN] = s.lost;
    tally[wave][kTruncated] = s.truncated;
    tally[wave][kSampleLo] = (unsigned)s.sync_sample;
    tally[wave][kSampleHi] = (unsigned)(s.sync_sample >> 32);
    lastsum[wave][0] = s.sum[0][0];
    lastsum[wave][1] = s.sum[0][1];
    lastsum[wave][2] = s.sum[1][0];
    lastsum[wave][3] = s.sum[1][1];
  }
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
      for (int i = 0; i < W; i++)  // side by side, as k_rtty and k_dsc have them
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
      for (int i = 0; i < done; i++) {  // the header's step, frame k0 + i
        s.frames = sat_inc(s.frames);
        s.t -= 256;
        if (s.t >= 128) continue;
        unsigned long long const Pm = Pb[wave][0][i], Ps = Pb[wave][1][i], hi = Pm >= Ps ? Pm : Ps, lo = Pm >= Ps ? Ps : Pm;
        if (s.ph == 0) {
          s.pe = hi;
          s.t += q;
          s.ph = 1;
        } else if (s.ph == 1) {
          s.bit = Pm >= Ps ? 1u : 0u;
          s.hi = hi;
          s.lo = lo;
          s.t += q;
          s.ph = 2;
        } else {
          s.ph = 0;
          bit_step(g, w.par, s, hi, (unsigned long long)(pc.k0 + i), ev, nev, tally[wave]);
        }
      }
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  __syncthreads();
  tc::store_hist(A[wave], c.hist, w);
  if (w.live && lane == 0) {
    s.syncs = tally[wave][kSyncs];
    s.eoms = tally[wave][kEoms];
    s.complete = tally[wave][kCompleteN];
    s.lost = tally[wave][kLostN];
    s.truncated = tally[wave][kTruncated];
    s.sync_sample = (unsigned long long)tally[wave][kSampleHi] << 32 | tally[wave][kSampleLo];
    s.sum[0][0] = lastsum[wave][0];
    s.sum[0][1] = lastsum[wave][1];
    s.sum[1][0] = lastsum[wave][2];
    s.sum[1][1] = lastsum[wave][3];
  }
  s.acc[0][0] = cy[0];
  s.acc[0][1] = cy[1];
  s.acc[1][0] = cy[2];
  s.acc[1][1] = cy[3];
  tc::store_record(c, w, s, nev);
}

}  // namespace

struct kq_same_bank : tc::GridBank<SameKind> {};

extern "C" {

kq_same_bank *kq_same_create(const kq_same_config *cfg) {
  const char *fn = "kq_same_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !kq::field_in_range(fn, "sync_errs", cfg->sync_errs, 0, 4) ||
      !kq::field_in_range(fn, "lose", cfg->lose, 1, 15) || !kq::field_in_range(fn, "max_len", cfg->max_len, 8, 248) ||
      !tc::config_tail_ok(fn, cfg, kMaxSlots))
    return nullptr;
  kq_same_bank *b = tc::finish_create<kq_same_bank>(cfg, kTile);  // Lmin 8 at the most: Bs <= 258
  b->g.sync_errs = cfg->sync_errs;
  b->g.lose = cfg->lose;
  b->g.max_len = cfg->max_len;
  return b;
}

int kq_same_destroy(kq_same_bank *b) { return kq::destroy_bank(b, "kq_same_destroy"); }

int kq_same_set(kq_same_bank *b, unsigned slot, const kq_same_params *p) {
  const char *fn = "kq_same_set";
  std::unique_lock<std::mutex> lk;
  if (!tc::open_set(b, fn, slot, p, kMaxSlots, lk)) return -1;
  double const Fs = b->cfg.samprate;
  SamePar np{};
  if (!tc::tone_pair(fn, Fs, p->mark, p->space, &np.inc_m, &np.inc_s) ||
      !tc::symbol_period(fn, Fs, b->cfg.block_len, p->baud, "bit", &np.tb, &np.W))
    return -1;
  np.active = 1;
  np.source = p->source;
  b->def.set(slot, np);
  return 0;
}

int kq_same_remove(kq_same_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_same_remove"); }

int kq_same_process(kq_same_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_same_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_same_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL(k_same, dim3(blocks), dim3(kThreads), 0, b->stream, a);
                               });
}

int kq_same_pull_counts(kq_same_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_same_pull_counts", counts); }

int kq_same_pull_event(kq_same_bank *b, unsigned slot, unsigned index, kq_same_event *event) {
  return kq::pull_event(b, "kq_same_pull_event", slot, index, event);
}

int kq_same_clear_events(kq_same_bank *b) { return kq::clear_arena(b, "kq_same_clear_events"); }

int kq_same_get_table(const kq_same_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_same_get_table", dst, cap);
}

int kq_same_get_slot(kq_same_bank *b, unsigned slot, kq_same_slot *out) {
  std::unique_lock<std::mutex> lk;
  const SamePar *w = tc::wanted(b, "kq_same_get_slot", slot, out, "out", lk);
  if (!w) return -1;
  tc::get_pair_slot(*w, out);
  return 0;
}

int kq_same_sync(kq_same_bank *b) { return kq::sync_bank(b, "kq_same_sync"); }

int kq_same_reset(kq_same_bank *b) { return kq::deferred_reset(b, "kq_same_reset"); }

}  // extern "C"
