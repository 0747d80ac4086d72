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
// k_same    the tracker above the bit, and the name of its instance of bc::bit_clock (kq_bitclock.hpp), the kernel k_dsc
//           and k_navtex run in too.  The format is ASCII behind a fixed preamble, so the device needs no table: two 48-bit
//           patterns and a range test.  There is no open message: the whole record, 49 words, travels through lane 0
//           (bc::WholeRecord).  It is a word longer than k_navtex's, which sat on the bound of 128 VGPRs, so what a bit
//           seldom touches waits in LDS between the load and the store and not in lane 0's registers (kParks): the five
//           burst counters and sync_sample (tally, 28 bytes a wave) and the window sums of the last completed frame
//           (the kernel's lastsum, which it has anyway).
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

// the bank's types for tc::GridBank, and its tracker for bc::bit_clock
struct k_same : bc::WholeRecord {
  using Config = kq_same_config;
  using Geom = SameGeom;
  using Par = tc::PairPar;
  using Status = kq_same_status;
  using Event = kq_same_event;
  using Hist = tc::FrameHist<4>;  // a, b of mark, a, b of space
  using Tables = tc::NoTables;
  static constexpr bool kZeroCold = true;
  using Side = unsigned[kTally];  // what a bit seldom touches (see the top)
  static constexpr bool kParks = true;

  static __device__ void park(kq_same_status const &s, Side (&tally)[bc::kWaves], int wave);
  static __device__ void unpark(kq_same_status &s, Side (&tally)[bc::kWaves], int wave);
  static __device__ void bit_step(SameGeom const &g, Par const &par, kq_same_status &s, Side &tally, unsigned long long pl,
                                  unsigned long long k, kq_same_event *ev, unsigned &nev);
};
using CallArgs = tc::GridBank<k_same>::Args;

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

__device__ __forceinline__ void k_same::park(kq_same_status const &s, Side (&tally)[bc::kWaves], int wave) {
  tally[wave][kSyncs] = s.syncs;
  tally[wave][kEoms] = s.eoms;
  tally[wave][kCompleteN] = s.complete;
  tally[wave][kLostN] = s.lost;
  tally[wave][kTruncated] = s.truncated;
  tally[wave][kSampleLo] = (unsigned)s.sync_sample;
  tally[wave][kSampleHi] = (unsigned)(s.sync_sample >> 32);
}

__device__ __forceinline__ void k_same::unpark(kq_same_status &s, Side (&tally)[bc::kWaves], int wave) {
  s.syncs = tally[wave][kSyncs];
  s.eoms = tally[wave][kEoms];
  s.complete = tally[wave][kCompleteN];
  s.lost = tally[wave][kLostN];
  s.truncated = tally[wave][kTruncated];
  s.sync_sample = (unsigned long long)tally[wave][kSampleHi] << 32;  // (in two statements: as one expression, in a
  s.sync_sample |= tally[wave][kSampleLo];                           // function, it compiles to another listing)
}

// the header's steps 1 to 5: the late point of a bit at frame k, with the late power pl
__device__ __forceinline__ void k_same::bit_step(SameGeom const &g, tc::PairPar const &par, kq_same_status &s, Side &tally,
                                         unsigned long long pl, unsigned long long k, kq_same_event *ev, unsigned &nev) {
  bool const open = tc::bit_levels(g, par, s, pl);  // 1 timing, 2 levels and gate
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

}  // namespace

struct kq_same_bank : tc::GridBank<k_same> {};

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
  kq_same_bank *b = tc::finish_create<kq_same_bank>(cfg, bc::kTile);  // Lmin 8 at the most: Bs <= 258
  b->g.sync_errs = cfg->sync_errs;
  b->g.lose = cfg->lose;
  b->g.max_len = cfg->max_len;
  return b;
}

int kq_same_destroy(kq_same_bank *b) { return kq::destroy_bank(b, "kq_same_destroy"); }

int kq_same_set(kq_same_bank *b, unsigned slot, const kq_same_params *p) {
  return tc::set_pair(b, "kq_same_set", slot, p, kMaxSlots);
}

int kq_same_remove(kq_same_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_same_remove"); }

int kq_same_process(kq_same_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_same_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_same_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, bc::kWaves, [b](CallArgs &a, unsigned blocks) {
                                 hipLaunchKernelGGL((bc::bit_clock<k_same, CallArgs>), dim3(blocks), dim3(bc::kThreads), 0,
                                                    b->stream, a);
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
  return tc::get_pair(b, "kq_same_get_slot", slot, out);
}

int kq_same_sync(kq_same_bank *b) { return kq::sync_bank(b, "kq_same_sync"); }

int kq_same_reset(kq_same_bank *b) { return kq::deferred_reset(b, "kq_same_reset"); }

}  // extern "C"
