// kq_navtex.hip -- NAVTEX / SITOR-B (CCIR 476 collective B mode, forward error correction by time diversity) decoder bank:
// the audio of SSB channels -> one event per character (the code, flags, the DX and the RX word, end, sig, nse) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_navtex_*): kq_dsc_*'s front half and bit clock to the letter -- quantise, correlate every
// frame of B samples against the mark and the space tone, slide a window one bit long over the frames' reduced sums, step
// the three-point clock once per completed frame -- and at every third point of the clock a bit is read: the levels, the
// gate, the 128-bit register, and -- at every bit while there is no sync -- the attempt on the phasing signals and, where
// that fails, on the agreement of the two copies in running traffic, on the register and on its complement; in sync, at
// every seventh bit a place, and at every RX place a character resolved from its DX copy in bits 41..35 or its RX copy in
// bits 6..0.  All exact integers after the quantiser.  State on the device, per slot: one kq_navtex_status record, the
// reduced sums of the last 31 frames, and the arena of events; per bank the table.  The signal format and the alphabet are
// written down from memory (the header says what is and what is not verified).
//
// k_navtex  the tracker above the bit, and the name of its instance of bc::bit_clock (kq_bitclock.hpp), the kernel k_dsc
//           runs in too.  A seven-bit word is a character if four of its bits are B, so the device needs no table of the
//           alphabet: alpha, beta and rep are the three words it knows by name.  There is no open message: the whole
//           record, 48 words, travels through lane 0 (bc::WholeRecord), and the wave keeps no LDS beyond the kernel's own.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

#include "ka9q_hip.h"
#include "kq_bitclock.hpp"

namespace tc = kq::tonecorr;
namespace bc = kq::bitclock;

namespace {

using tc::sat_inc;
constexpr unsigned kMaxSlots = 16384;
constexpr unsigned kAlpha = 0x78, kBeta = 0x66, kRep = 0x33;  // BBBBYYY, BBYYBBY, YBBYYBB: the first bit sent in bit 6
constexpr unsigned kNone = 0x7F;                // the code of a character neither copy gave
constexpr unsigned kUnresolved = 1, kFromRx = 2, kDiffer = 4, kInverted = 8;
constexpr int kPairs = 6;                       // pairs of copies the register holds: 14 * 5 + 41 < 128

struct NavtexGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr, acq, pairs, lose;
  unsigned long long min_p;
  int max_events;
};

// the bank's types for tc::GridBank, and its tracker for bc::bit_clock
struct k_navtex : bc::WholeRecord {
  using Config = kq_navtex_config;
  using Geom = NavtexGeom;
  using Par = tc::PairPar;
  using Status = kq_navtex_status;
  using Event = kq_navtex_event;
  using Hist = tc::FrameHist<4>;  // a, b of mark, a, b of space
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
  using Side = bc::NoSide;        // there is no open message: the whole record travels through lane 0
  static constexpr bool kParks = false;

  static __device__ void bit_step(NavtexGeom const &g, Par const &par, kq_navtex_status &s, Side &, unsigned long long pl,
                                  unsigned long long k, kq_navtex_event *ev, unsigned &nev);
};
using CallArgs = tc::GridBank<k_navtex>::Args;

// the constant-ratio code: four of seven bits are B
__device__ __forceinline__ bool is_char(unsigned w) { return __popc(w) == 4; }

// the seven bits at..at + 6 of the register (hi, lo); `at` is a constant once the callers' loops are unrolled
__device__ __forceinline__ unsigned word_at(unsigned long long hi, unsigned long long lo, int at) {
  unsigned long long v = at >= 64 ? hi >> (at - 64) : lo >> at;
  if (at > 57 && at < 64) v |= hi << (64 - at);
  return (unsigned)v & 127u;
}

// step 4, the phasing signals on x (its low 28 bits): 1 the latest place is RX, 0 it is DX, -1 no sync
__device__ __forceinline__ int phasing(unsigned long long x, unsigned acq) {
  unsigned const c0 = (unsigned)x & 127u, c1 = (unsigned)(x >> 7) & 127u, c2 = (unsigned)(x >> 14) & 127u,
                 c3 = (unsigned)(x >> 21) & 127u;
  unsigned const as_rx = (unsigned)(c0 == kAlpha) + (unsigned)(c1 == kRep) + (unsigned)(c2 == kAlpha) + (unsigned)(c3 == kRep);
  unsigned const as_dx = (unsigned)(c0 == kRep) + (unsigned)(c1 == kAlpha) + (unsigned)(c2 == kRep) + (unsigned)(c3 == kAlpha);
  return as_rx >= acq ? 1 : as_dx >= acq ? 0 : -1;
}

// step 4, running traffic on x = (hi, lo): the first `pairs` pairs each hold two equal characters, none of them alpha,
// beta or rep, and not all pairs the same character
__device__ __forceinline__ bool traffic(unsigned long long hi, unsigned long long lo, unsigned pairs) {
  bool ok = true, two = false;
  unsigned const first = (unsigned)lo & 127u;
#pragma unroll
  for (int j = 0; j < kPairs; j++) {
    unsigned const rx = word_at(hi, lo, 14 * j), dx = word_at(hi, lo, 14 * j + 35);
    bool const good = rx == dx && is_char(rx) && rx != kAlpha && rx != kBeta && rx != kRep;
    if ((unsigned)j < pairs) {
      ok = ok && good;
      two = two || rx != first;
    }
  }
  return ok && two;
}

__device__ __forceinline__ void file(NavtexGeom const &g, kq_navtex_status &s, unsigned code, unsigned flags, unsigned dx,
                                     unsigned rx, unsigned long long k, kq_navtex_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_navtex_event &r = ev[nev++];
  r.code = code;
  r.flags = flags | (s.inverted ? kInverted : 0u);
  r.dx = dx;
  r.rx = rx;
  r.end_sample = (k + 1) * (unsigned long long)g.grid.B;
  r.sig = s.sig;
  r.nse = s.nse;
}

// the header's steps 1 to 5: the late point of a bit at frame k, with the late power pl
__device__ __forceinline__ void k_navtex::bit_step(NavtexGeom const &g, tc::PairPar const &par, kq_navtex_status &s, bc::NoSide &,
                                         unsigned long long pl, unsigned long long k, kq_navtex_event *ev, unsigned &nev) {
  bool const open = tc::bit_levels(g, par, s, pl);  // 1 timing, 2 levels and gate
  // 3 register
  s.r_hi = s.r_hi << 1 | s.r_lo >> 63;
  s.r_lo = s.r_lo << 1 | (unsigned long long)s.bit;
  s.nbits += 1;
  // 4 sync
  if (!s.synced) {
    if (!open) return;
    int kind = phasing(s.r_lo, g.acq);
    unsigned inv = 0, by_traffic = 0;
    if (kind < 0 && traffic(s.r_hi, s.r_lo, g.pairs)) kind = 1, by_traffic = 1;
    if (kind < 0) {
      inv = 1;
      kind = phasing(~s.r_lo, g.acq);
      if (kind < 0 && traffic(~s.r_hi, ~s.r_lo, g.pairs)) kind = 1, by_traffic = 1;
    }
    if (kind < 0) return;
    s.synced = 1;
    s.bitpos = 0;
    s.kind = (unsigned)kind;
    s.inverted = inv;
    s.run = 0;
    if (by_traffic) s.tsyncs = sat_inc(s.tsyncs);
    else s.syncs = sat_inc(s.syncs);
    return;
  }
  // 5 characters
  s.bitpos += 1;
  if (s.bitpos < 7) return;
  s.bitpos = 0;
  s.kind ^= 1u;
  if (!s.kind) return;
  unsigned long long const x = s.inverted ? ~s.r_lo : s.r_lo;
  unsigned const dx = (unsigned)(x >> 35) & 127u, rx = (unsigned)x & 127u;
  bool const by_dx = is_char(dx), by_rx = is_char(rx);
  bool const clean = (dx == kRep && rx == kAlpha) || (by_dx && by_rx && dx == rx);
  s.run = clean ? 0u : s.run + 1;
  if (dx == kRep || rx == kAlpha) {
    s.idles = sat_inc(s.idles);
  } else {
    unsigned const code = by_dx ? dx : by_rx ? rx : kNone;
    unsigned const flags = by_dx ? (by_rx && rx != dx ? kDiffer : 0u) : by_rx ? kFromRx : kUnresolved;
    file(g, s, code, flags, dx, rx, k, ev, nev);
  }
  if (s.run >= g.lose) {
    s.synced = 0;
    s.losses = sat_inc(s.losses);
  }
}

}  // namespace

struct kq_navtex_bank : tc::GridBank<k_navtex> {};

extern "C" {

kq_navtex_bank *kq_navtex_create(const kq_navtex_config *cfg) {
  const char *fn = "kq_navtex_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !kq::field_in_range(fn, "acq", cfg->acq, 3, 4) ||
      !kq::field_in_range(fn, "pairs", cfg->pairs, 3, kPairs) || !kq::field_in_range(fn, "lose", cfg->lose, 1, 255) ||
      !tc::config_tail_ok(fn, cfg, kMaxSlots))
    return nullptr;
  kq_navtex_bank *b = tc::finish_create<kq_navtex_bank>(cfg, bc::kTile);  // Lmin 8 at the most: Bs <= 258
  b->g.acq = cfg->acq;
  b->g.pairs = cfg->pairs;
  b->g.lose = cfg->lose;
  return b;
}

int kq_navtex_destroy(kq_navtex_bank *b) { return kq::destroy_bank(b, "kq_navtex_destroy"); }

int kq_navtex_set(kq_navtex_bank *b, unsigned slot, const kq_navtex_params *p) {
  return tc::set_pair(b, "kq_navtex_set", slot, p, kMaxSlots);
}

int kq_navtex_remove(kq_navtex_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_navtex_remove"); }

int kq_navtex_process(kq_navtex_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                      unsigned nblocks, int on_device, kq_navtex_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_navtex_process", src, format, src_stride, row_stride, block_len, nblocks, on_device,
                               status, status_stride, bc::kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL((bc::bit_clock<k_navtex, CallArgs>), dim3(blocks), dim3(bc::kThreads), 0,
                                                    b->stream, a);
                               });
}

int kq_navtex_pull_counts(kq_navtex_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_navtex_pull_counts", counts); }

int kq_navtex_pull_event(kq_navtex_bank *b, unsigned slot, unsigned index, kq_navtex_event *event) {
  return kq::pull_event(b, "kq_navtex_pull_event", slot, index, event);
}

int kq_navtex_clear_events(kq_navtex_bank *b) { return kq::clear_arena(b, "kq_navtex_clear_events"); }

int kq_navtex_get_table(const kq_navtex_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_navtex_get_table", dst, cap);
}

int kq_navtex_get_slot(kq_navtex_bank *b, unsigned slot, kq_navtex_slot *out) {
  return tc::get_pair(b, "kq_navtex_get_slot", slot, out);
}

int kq_navtex_sync(kq_navtex_bank *b) { return kq::sync_bank(b, "kq_navtex_sync"); }

int kq_navtex_reset(kq_navtex_bank *b) { return kq::deferred_reset(b, "kq_navtex_reset"); }

}  // extern "C"
