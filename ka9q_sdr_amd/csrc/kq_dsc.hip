// kq_dsc.hip -- GMDSS digital selective calling (ITU-R M.493) decoder bank: the audio of SSB channels (or of a flat FM
// channel at 96 kHz) -> whole DSC messages, as events (the symbols, nsym, flags, holes, from_rx, hole_mask, sync and end,
// sig, nse) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_dsc_*): quantise as kq_cw_*, correlate every frame of B samples against the mark and the
// space tone from the 1024-entry cosine table with phases that are functions of the sample index alone, slide a window one
// bit long (W frames) over the frames' reduced sums -- kq_rtty_*'s front half to the letter -- and step the bit clock once
// per completed frame; at every third point of the clock a bit is read: the levels, the gate, the 64-bit register, and --
// at every bit while there is no sync -- the attempt on the phasing sequence, on the register and on its complement; in
// sync, at every tenth bit a symbol place, and at every odd place from 17 on a message symbol resolved from its DX copy in
// bits 59..50 or its RX copy in bits 9..0.  All exact integers after the quantiser.  State on the device, per slot: one
// kq_dsc_status record, the reduced sums of the last 31 frames, and the arena of events; per bank the table.  The signal
// format is written down from memory (the header says what is and what is not verified).
//
// k_dsc   the tracker above the bit, and the name of its instance of bc::bit_clock (kq_bitclock.hpp: the frame-grid kernel
//         with a window and a bit clock, two tones, four series, as k_rtty; lane 0 walks the piece's (Pm, Ps) pairs in order
//         through the clock).  The symbol code is a popcount and a bit reversal, so the tracker has no table.  The record's
//         tail, the open message (kq_dsc_message: 64 bytes written at a running index, and the counts beside them that
//         change once in ten bits), goes from the device's memory to LDS and back by the wave's first lanes and never
//         through lane 0's registers: there the index would put it in scratch, and its 30 words beside the 40 of the head
//         would cost the fourth workgroup of a CU.
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
constexpr int kMsg = 64;                        // symbols to a message at the most
constexpr unsigned kW125 = 0x2F9;               // symbol 125 as sent: 1011111001
constexpr unsigned kCheck = 1, kTruncated = 2, kLost = 4, kInverted = 8;

struct DscGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr, acq, lose;
  unsigned long long min_p;
  int max_events;
};

// the bank's types for tc::GridBank, and its tracker for bc::bit_clock
struct k_dsc {
  using Config = kq_dsc_config;
  using Geom = DscGeom;
  using Par = tc::PairPar;
  using Status = kq_dsc_status;
  using Event = kq_dsc_event;
  using Hist = tc::FrameHist<4>;  // a, b of mark, a, b of space
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
  using Side = kq_dsc_message;    // the record's tail, the open message
  static constexpr bool kParks = false;

  template <class Args, class Place>
  static __device__ kq_dsc_event *load(Args const &c, Place const &w, kq_dsc_status &s, Side (&side)[bc::kWaves], unsigned &nev);
  template <class Args, class Place>
  static __device__ void store(Args const &c, Place const &w, kq_dsc_status const &s, Side (&side)[bc::kWaves], unsigned nev);
  static __device__ void bit_step(DscGeom const &g, Par const &par, kq_dsc_status &s, kq_dsc_message &m, unsigned long long pl,
                                  unsigned long long k, kq_dsc_event *ev, unsigned &nev);
};
using CallArgs = tc::GridBank<k_dsc>::Args;

// the symbol code: a ten-bit word, its first bit sent in bit 9
__device__ __forceinline__ bool is_symbol(unsigned w) { return 7u - (unsigned)__popc(w >> 3) == (w & 7u); }
__device__ __forceinline__ unsigned value_of(unsigned w) { return __brev(w >> 3) >> 25; }
__device__ __forceinline__ unsigned word_of(unsigned v) { return (__brev(v) >> 25) << 3 | (7u - (unsigned)__popc(v)); }

// step 4 on x: the place of the latest symbol, or -1
__device__ __forceinline__ int phasing(unsigned long long x, unsigned acq) {
  unsigned const s0 = (unsigned)x & 1023u, s1 = (unsigned)(x >> 10) & 1023u, s2 = (unsigned)(x >> 20) & 1023u,
                 s3 = (unsigned)(x >> 30) & 1023u;
  if (!is_symbol(s0)) return -1;
  unsigned const v = value_of(s0);
  if (v < 104 || v > 110) return -1;
  unsigned const m = (unsigned)(s2 == word_of(v + 1)) + (unsigned)(v >= 106 && s1 == kW125) + (unsigned)(v >= 105 && s3 == kW125);
  return m >= acq ? (int)(2 * (111 - v) + 1) : -1;
}

__device__ __forceinline__ void file(DscGeom const &g, kq_dsc_status &s, kq_dsc_message const &m, unsigned flags,
                                     unsigned long long k, kq_dsc_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_dsc_event &r = ev[nev++];
  unsigned *sym = reinterpret_cast<unsigned *>(r.sym);
  const unsigned *msg = reinterpret_cast<const unsigned *>(m.msg);
#pragma unroll
  for (int i = 0; i < kMsg / 4; i++) sym[i] = msg[i];
  r.nsym = m.nsym;
  r.flags = flags | (m.inverted ? kInverted : 0u);
  r.holes = m.holes;
  r.from_rx = m.from_rx;
  r.hole_mask = m.hole_mask;
  r.sync_sample = m.sync_sample;
  r.end_sample = (k + 1) * (unsigned long long)g.grid.B;
  r.sig = s.sig;
  r.nse = s.nse;
}

constexpr int kHead = (int)offsetof(kq_dsc_status, open), kOpenWords = (int)sizeof(kq_dsc_message) / 4;
static_assert(kHead % 8 == 0 && sizeof(kq_dsc_message) % 8 == 0 && kOpenWords <= 64, "the record's head and its tail");

// the header's steps 1 to 5: the late point of a bit at frame k, with the late power pl; m: the open message, in LDS
__device__ __forceinline__ void k_dsc::bit_step(DscGeom const &g, tc::PairPar const &par, kq_dsc_status &s, kq_dsc_message &m,
                                         unsigned long long pl, unsigned long long k, kq_dsc_event *ev, unsigned &nev) {
  bool const open = tc::bit_levels(g, par, s, pl);  // 1 timing, 2 levels and gate
  // 3 register
  s.r = s.r << 1 | (unsigned long long)s.bit;
  s.nbits += 1;
  // 4 sync
  if (!s.synced) {
    if (!open) return;
    int place = phasing(s.r, g.acq);
    unsigned inv = 0;
    if (place < 0) {
      place = phasing(~s.r, g.acq);
      inv = 1;
    }
    if (place < 0) return;
    s.synced = 1;
    s.bitpos = 0;
    s.syncs = sat_inc(s.syncs);
    m.inverted = inv;
    m.place = (unsigned)place;
    m.nsym = m.nres = m.holes = m.from_rx = m.run = m.ecc = m.eos = 0;
    m.hole_mask = 0;
    m.sync_sample = (k + 1) * (unsigned long long)g.grid.B;
    unsigned *msg = reinterpret_cast<unsigned *>(m.msg);
#pragma unroll
    for (int i = 0; i < kMsg / 4; i++) msg[i] = 0;
    return;
  }
  // 5 message
  s.bitpos += 1;
  if (s.bitpos < 10) return;
  s.bitpos = 0;
  unsigned const place = m.place + 1;
  m.place = place;
  if (!(place & 1u) || place < 17) return;
  unsigned const i = (place - 17) >> 1;  // below kMsg: rule (b) ends the message at 64
  unsigned long long const x = m.inverted ? ~s.r : s.r;
  unsigned const dx = (unsigned)(x >> 50) & 1023u, rx = (unsigned)x & 1023u;
  bool const by_dx = is_symbol(dx), by_rx = is_symbol(rx), got = by_dx || by_rx;
  unsigned const d = by_dx ? value_of(dx) : value_of(rx);
  if (!by_dx && by_rx) m.from_rx += 1;
  m.msg[i & (kMsg - 1)] = (unsigned char)(got ? d : 0xFFu);
  m.nsym = i + 1;
  if (!got) {
    m.holes += 1;
    m.hole_mask |= 1ull << (i & 63u);
  }
  if (m.eos) {  // (a) the error-check symbol
    file(g, s, m, !got || m.holes || d != m.ecc ? kCheck : 0u, k, ev, nev);
    s.synced = 0;
    return;
  }
  if (!got) {
    m.run += 1;
    if (m.run >= g.lose) {  // (c)
      if (m.nres >= 8) file(g, s, m, kLost | kCheck, k, ev, nev);
      else s.aborted = sat_inc(s.aborted);
      s.synced = 0;
      return;
    }
  } else {
    m.run = 0;
    m.nres += 1;
    if (i >= 1) m.ecc ^= d;
    if (d == 117 || d == 122 || d == 127) m.eos = 1;
  }
  if (i + 1 == kMsg) {  // (b)
    file(g, s, m, kTruncated | kCheck, k, ev, nev);
    s.synced = 0;
  }
}

// tc::load_record and tc::store_record for a record in two parts: the head into lane 0, the tail (the open message) into
// LDS by the wave's first lanes
template <class Args, class Place>
__device__ __forceinline__ kq_dsc_event *k_dsc::load(Args const &c, Place const &w, kq_dsc_status &s, Side (&side)[bc::kWaves],
                                                     unsigned &nev) {
  kq_dsc_message &m = side[w.wave];
  if (w.live && w.lane == 0) {
    __builtin_memcpy(&s, &c.state[w.slot], kHead);
    nev = c.nev[w.slot];
  }
  if (w.lane < kOpenWords)
    reinterpret_cast<unsigned *>(&m)[w.lane] = w.live ? reinterpret_cast<const unsigned *>(&c.state[w.slot].open)[w.lane] : 0u;
  return c.ev + (size_t)w.slot * c.g.max_events;
}

template <class Args, class Place>
__device__ __forceinline__ void k_dsc::store(Args const &c, Place const &w, kq_dsc_status const &s, Side (&side)[bc::kWaves],
                                             unsigned nev) {
  kq_dsc_message const &m = side[w.wave];
  if (!w.live) return;
  kq_dsc_status *const out = c.st ? c.st + (size_t)w.slot * c.sstride : nullptr;
  if (w.lane == 0) {
    __builtin_memcpy(&c.state[w.slot], &s, kHead);
    c.nev[w.slot] = nev;
    if (out) __builtin_memcpy(out, &s, kHead);
  }
  if (w.lane < kOpenWords) {
    unsigned const v = reinterpret_cast<const unsigned *>(&m)[w.lane];
    reinterpret_cast<unsigned *>(&c.state[w.slot].open)[w.lane] = v;
    if (out) reinterpret_cast<unsigned *>(&out->open)[w.lane] = v;
  }
}

}  // namespace

struct kq_dsc_bank : tc::GridBank<k_dsc> {};

extern "C" {

kq_dsc_bank *kq_dsc_create(const kq_dsc_config *cfg) {
  const char *fn = "kq_dsc_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !kq::field_in_range(fn, "acq", cfg->acq, 1, 3) ||
      !kq::field_in_range(fn, "lose", cfg->lose, 1, 15) || !tc::config_tail_ok(fn, cfg, kMaxSlots))
    return nullptr;
  kq_dsc_bank *b = tc::finish_create<kq_dsc_bank>(cfg, bc::kTile);  // Lmin 8 at the most: Bs <= 258
  b->g.acq = cfg->acq;
  b->g.lose = cfg->lose;
  return b;
}

int kq_dsc_destroy(kq_dsc_bank *b) { return kq::destroy_bank(b, "kq_dsc_destroy"); }

int kq_dsc_set(kq_dsc_bank *b, unsigned slot, const kq_dsc_params *p) {
  return tc::set_pair(b, "kq_dsc_set", slot, p, kMaxSlots);
}

int kq_dsc_remove(kq_dsc_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_dsc_remove"); }

int kq_dsc_process(kq_dsc_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_dsc_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_dsc_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, bc::kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL((bc::bit_clock<k_dsc, CallArgs>), dim3(blocks), dim3(bc::kThreads), 0,
                                                    b->stream, a);
                               });
}

int kq_dsc_pull_counts(kq_dsc_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_dsc_pull_counts", counts); }

int kq_dsc_pull_event(kq_dsc_bank *b, unsigned slot, unsigned index, kq_dsc_event *event) {
  return kq::pull_event(b, "kq_dsc_pull_event", slot, index, event);
}

int kq_dsc_clear_events(kq_dsc_bank *b) { return kq::clear_arena(b, "kq_dsc_clear_events"); }

int kq_dsc_get_table(const kq_dsc_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_dsc_get_table", dst, cap);
}

int kq_dsc_get_slot(kq_dsc_bank *b, unsigned slot, kq_dsc_slot *out) { return tc::get_pair(b, "kq_dsc_get_slot", slot, out); }

int kq_dsc_sync(kq_dsc_bank *b) { return kq::sync_bank(b, "kq_dsc_sync"); }

int kq_dsc_reset(kq_dsc_bank *b) { return kq::deferred_reset(b, "kq_dsc_reset"); }

}  // extern "C"
