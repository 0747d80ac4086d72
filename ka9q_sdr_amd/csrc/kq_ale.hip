// kq_ale.hip -- HF ALE (MIL-STD-188-141 Appendix A, 8-FSK) decoder bank: the audio of USB channels -> 24-bit ALE words, as
// events (word, flags, err_a, err_b, split, end, sig, nse) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_ale_*): quantise as kq_cw_*, correlate every frame of B samples against eight tones from
// the 1024-entry cosine table with phases that are functions of the sample index alone, slide a window one symbol long (W
// frames) over the frames' reduced sums, take the largest of the eight powers, and step the symbol clock once per
// completed frame; at every third point of the clock a symbol is read: the levels, the gate, the 147-bit register, and --
// at every symbol while there is no word sync, at every 49th while there is -- the word attempt: majority vote over the
// three copies, de-interleave, Golay (24,12) by two 4096-entry tables.  All exact integers after the quantiser.  State on
// the device, per slot: one kq_ale_status record, the reduced sums of the last 31 frames, and the arena of events; per bank
// the cosine table and the two Golay tables.  The signal format is written down from memory (the header says what is and
// what is not verified); golay_parity() below is the single statement of the code, as PARITY is in ka9q_sdr_amd/ale2g.py.
//
// k_ale   a frame-grid kernel with a window and a symbol clock (kq_tonecorr.hpp describes the mapping): eight tones,
//         sixteen series.  The window sums are spread over the wave, a (frame, tone, I / Q) to a lane at a time -- rows of
//         kRow words with kRow = 2 mod 32, so that the sixteen series of two neighbouring frames fall into 32 banks -- and
//         lane f then squares frame f's eight pairs and keeps the largest power, its tone and the others' sum.  Lane 0
//         walks the piece's frames in order through the clock: it reads LDS at the points only.  Both Golay tables sit in
//         LDS (16 KiB), because a slot without word sync looks into them at every symbol and the walk is serial.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

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
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50
constexpr int kRow = 98;                        // a wave's reduced sums of one kind: the history, a piece's 64 frames and pad
constexpr int kWin = 66;                        // a wave's window sums of one kind over a piece
constexpr int NT = 8, NS = 2 * NT;              // tones; series (I and Q of each)
constexpr int kGolay = 4096;
constexpr unsigned long long kM49 = (1ull << 49) - 1;

// the code: the 12 check bits of 12 data bits -- the remainder of data x^11 by g(x) = 0xC75, then the overall parity bit
unsigned golay_parity(unsigned d) {
  unsigned r = d << 11;
  for (int i = 22; i >= 11; i--)
    if (r >> i & 1) r ^= 0xC75u << (i - 11);
  return r << 1 | ((unsigned)(__builtin_popcount(d) + __builtin_popcount(r)) & 1u);
}

// [0, 4096) the parity table; [4096, 8192) by syndrome: weight << 12 | the data bits of the one error pattern of weight <= 3
// with that syndrome, 4 << 12 where there is none.  Made once, at the first kq_ale_create.
std::vector<unsigned short> const &golay_tables() {
  static std::vector<unsigned short> const tables = [] {
    std::vector<unsigned short> t((size_t)2 * kGolay, (unsigned short)(4u << 12));
    for (unsigned d = 0; d < kGolay; d++) t[d] = (unsigned short)golay_parity(d);
    t[kGolay] = 0;
    for (int i = 0; i < 24; i++)
      for (int j = i; j < 24; j++)
        for (int k = j; k < 24; k++) {  // i == j or j == k give the lighter patterns
          unsigned const e = 1u << i | 1u << j | 1u << k;
          t[kGolay + (t[e >> 12] ^ (e & 0xFFFu))] = (unsigned short)((unsigned)__builtin_popcount(e) << 12 | e >> 12);
        }
    return t;
  }();
  return tables;
}

struct AleGeom {
  kq::tonecorr::FrameGrid grid;
  unsigned warm, snr, acq_err, lose;
  unsigned long long min_p;
  int max_events;
};

struct AlePar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc[NT];
  int tb, W;
};

struct AleTables {  // the bank's own, beside the cosine table
  unsigned short *golay = nullptr;  // [2][4096]
  int make(kq::HostSide &h) {       // (queued: the caller waits)
    if (h.alloc(&golay, (size_t)2 * kGolay)) return -1;
    KQ_TRY(hipMemcpyAsync(golay, golay_tables().data(), 2 * kGolay * sizeof(unsigned short), hipMemcpyHostToDevice, h.stream));
    return 0;
  }
};

struct AleKind {
  using Config = kq_ale_config;
  using Geom = AleGeom;
  using Par = AlePar;
  using Status = kq_ale_status;
  using Event = kq_ale_event;
  using Hist = tc::FrameHist<NS>;  // a, b of tone t at [2 t], [2 t + 1]
  using Tables = AleTables;
  static constexpr bool kZeroCold = true;
};

struct CallArgs : tc::GridBank<AleKind>::Args {
  const unsigned short *golay;
};

// bits 0, 2, .. 46 of x, packed
__device__ __forceinline__ unsigned even_bits(unsigned long long x) {
  x &= 0x5555555555555555ull;
  x = (x | x >> 1) & 0x3333333333333333ull;
  x = (x | x >> 2) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | x >> 4) & 0x00FF00FF00FF00FFull;
  x = (x | x >> 8) & 0x0000FFFF0000FFFFull;
  x = (x | x >> 16) & 0x00000000FFFFFFFFull;
  return (unsigned)x;
}

__device__ __forceinline__ bool in_set(unsigned c) {
  return (c >= '0' && c <= '9') || (c >= '@' && c <= 'Z') || c == '?';
}

__device__ __forceinline__ void file(AleGeom const &g, kq_ale_status &s, unsigned word, unsigned flags, unsigned ea, unsigned eb,
                                     unsigned split, unsigned long long k, kq_ale_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_ale_event r;
  r.word = word;
  r.flags = flags;
  r.err_a = ea;
  r.err_b = eb;
  r.split = split;
  r.reserved = 0;
  r.end_sample = (k + 1) * (unsigned long long)g.grid.B;
  r.sig = s.sig;
  r.nse = s.nse;
  ev[nev++] = r;
}

// the header's steps 1 to 5: the late point of a symbol at frame k, with the late power pl
__device__ __forceinline__ void symbol(AleGeom const &g, AlePar const &par, kq_ale_status &s, unsigned long long pl,
                                       unsigned long long k, const unsigned short *gol, kq_ale_event *ev, unsigned &nev) {
  // 1 timing
  tc::clock_adjust(s, par.tb, pl);
  // 2 levels and gate
  smooth(s.sig, s.pc, 4);
  smooth(s.nse, s.oth, 4);
  bool const gate = tc::gate16(s.sig, s.nse, g.snr), valid = s.frames >= g.warm && s.sig >= g.min_p && gate;
  // 3 register (the Gray map 0 1 3 2 6 7 5 4, a nibble to a tone)
  s.r0 = (s.r0 << 3 | s.r1 >> 46) & kM49;
  s.r1 = (s.r1 << 3 | s.r2 >> 46) & kM49;
  s.r2 = (s.r2 << 3 | (unsigned long long)((0x45762310u >> (4 * s.sym)) & 7u)) & kM49;
  s.nsym += 1;
  if (s.synced) s.wpos += 1;
  // 4 gate
  if (!valid) {
    s.synced = s.bad = s.wpos = 0;
    return;
  }
  // 5 word attempt
  if (s.synced && s.wpos < 49) return;
  unsigned long long const maj = (s.r0 & s.r1) | (s.r0 & s.r2) | (s.r1 & s.r2);
  if (!s.synced && (maj & 1)) return;  // (the stuff bit: nothing else of the attempt is kept)
  unsigned const split = (unsigned)__popcll((s.r0 ^ s.r1) | (s.r0 ^ s.r2));
  unsigned const A = even_bits(maj >> 2), Bh = even_bits(maj >> 1) ^ 0xFFFu;
  unsigned const xa = gol[kGolay + (gol[A >> 12] ^ (A & 0xFFFu))], xb = gol[kGolay + (gol[Bh >> 12] ^ (Bh & 0xFFFu))];
  unsigned const ea = xa >> 12, eb = xb >> 12;
  unsigned const word = ((A >> 12) ^ (xa & 0xFFFu)) << 12 | ((Bh >> 12) ^ (xb & 0xFFFu));
  if (!s.synced) {
    bool const chars = word >> 21 == 6u || (in_set(word >> 14 & 0x7Fu) && in_set(word >> 7 & 0x7Fu) && in_set(word & 0x7Fu));
    if (ea <= g.acq_err && eb <= g.acq_err && chars) {
      s.synced = 1;
      s.sync_at = s.nsym;
      s.wpos = s.bad = 0;
      file(g, s, word, 0, ea, eb, split, k, ev, nev);
    }
    return;
  }
  s.wpos = 0;
  if (ea < 4 && eb < 4) {
    s.bad = 0;
    file(g, s, word, 0, ea, eb, split, k, ev, nev);
  } else {
    file(g, s, word, 1, ea, eb, split, k, ev, nev);
    s.bad += 1;
    if (s.bad >= g.lose) s.synced = s.bad = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_ale(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ unsigned short GL[2 * kGolay];        // the parity table, then the error patterns by syndrome
  __shared__ __align__(16) unsigned char raw[kWaves][2 * kTile];  // a wave's samples; once they are correlated, its window sums
  __shared__ int A[kWaves][NS][kRow];              // reduced sums: [0, kHist) the frames before the piece, then the piece's
  __shared__ unsigned long long Pb[kWaves][64];    // the largest of the eight powers at every frame of the piece,
  __shared__ unsigned long long Ob[kWaves][64];    // the other seven, each >> 3, summed,
  __shared__ int Yb[kWaves][64];                   // and the tone
  __shared__ long long carry[kWaves][NS];
  __shared__ int lastsum[kWaves][NS];
  AleGeom const &g = c.g;
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane, W = tc::window_frames(w.live, w.par.W);
  for (int i = (int)threadIdx.x; i < kGolay; i += kThreads)  // two entries to a word
    reinterpret_cast<unsigned *>(GL)[i] = reinterpret_cast<const unsigned *>(c.golay)[i];
  int const q = w.par.tb >> 2;
  short *const qs = reinterpret_cast<short *>(raw[wave]);
  int(*const Wd)[kWin] = reinterpret_cast<int(*)[kWin]>(raw[wave]);  // [NS][kWin]: the window sums at every frame of the piece
  static_assert(NS * kWin * sizeof(int) <= 2 * kTile, "the window sums fit where the samples were");
  kq_ale_status s{};
  unsigned nev = 0;
  kq_ale_event *ev = tc::load_record(c, w, s, nev);
  long long cy[NS];
#pragma unroll
  for (int t = 0; t < NS; t++) cy[t] = 0;
  if (w.live && lane == 0) {
#pragma unroll
    for (int t = 0; t < NS; t++) {
      cy[t] = s.acc[t >> 1][t & 1];
      lastsum[wave][t] = s.sum[t >> 1][t & 1];
    }
  }
  tc::load_hist(A[wave], c.hist, w);
  for (tc::Piece pc(c.n0, w.B); pc.n < c.n1; pc.next(w.F)) {
    pc.span(c.n1, w.B, w.F);
    long long sm[NS];  // (its first barrier: the piece before is done with raw, A, Pb, Ob, Yb and carry, and A is loaded)
    tc::correlate_piece<NT>(c, w, pc, qs, CS, w.par.inc, sm, cy);
    int const done = pc.done(g.grid);
    tc::file_sums(A[wave], carry[wave], w, pc, done, sm, 12);
    __syncthreads();
    for (int it = lane; it < done * NS; it += 64) {  // series t at frame fr
      int const fr = it >> 4, t = it & (NS - 1);
      Wd[t][fr] = tc::window_sum(A[wave][t], fr, W);
    }
    __syncthreads();
    int keep[NS];
    tc::keep_hist(A[wave], lane, done, keep);
    if (lane < done) {
      unsigned long long best = 0, tot = 0;
      int sym = 0;
#pragma unroll
      for (int t = 0; t < NT; t++) {
        long long const wi = Wd[2 * t][lane], wq = Wd[2 * t + 1][lane];
        unsigned long long const P = (unsigned long long)(wi * wi) + (unsigned long long)(wq * wq);
        tot += P >> 3;
        if (P > best) {  // ties to the lowest tone
          best = P;
          sym = t;
        }
      }
      Pb[wave][lane] = best;
      Ob[wave][lane] = tot - (best >> 3);
      Yb[wave][lane] = sym;
      if (lane == done - 1)
#pragma unroll
        for (int t = 0; t < NS; t++) lastsum[wave][t] = Wd[t][lane];
    }
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
          s.sym = (unsigned)Yb[wave][i];
          s.pc = P;
          s.oth = Ob[wave][i];
          s.t += q;
          s.ph = 2;
        } else {
          s.ph = 0;
          symbol(g, w.par, s, P, (unsigned long long)(pc.k0 + i), GL, ev, nev);
        }
      }
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  __syncthreads();
  tc::store_hist(A[wave], c.hist, w);
  if (w.live && lane == 0) {
#pragma unroll
    for (int t = 0; t < NS; t++) {
      s.acc[t >> 1][t & 1] = cy[t];
      s.sum[t >> 1][t & 1] = lastsum[wave][t];
    }
  }
  tc::store_record(c, w, s, nev);
}

}  // namespace

struct kq_ale_bank : tc::GridBank<AleKind> {};

extern "C" {

kq_ale_bank *kq_ale_create(const kq_ale_config *cfg) {
  const char *fn = "kq_ale_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!tc::config_head_ok(fn, cfg) || !kq::field_in_range(fn, "acq_err", cfg->acq_err, 0, 3) ||
      !kq::field_in_range(fn, "lose", cfg->lose, 1, 15) || !tc::config_tail_ok(fn, cfg, kMaxSlots))
    return nullptr;
  (void)golay_tables();  // the tables exist from here on
  kq_ale_bank *b = tc::finish_create<kq_ale_bank>(cfg, kTile);  // Lmin 8 at the most: Bs <= 258
  b->g.acq_err = cfg->acq_err;
  b->g.lose = cfg->lose;
  return b;
}

int kq_ale_destroy(kq_ale_bank *b) { return kq::destroy_bank(b, "kq_ale_destroy"); }

int kq_ale_set(kq_ale_bank *b, unsigned slot, const kq_ale_params *p) {
  const char *fn = "kq_ale_set";
  std::unique_lock<std::mutex> lk;
  if (!tc::open_set(b, fn, slot, p, kMaxSlots, lk)) return -1;
  double const Fs = b->cfg.samprate, f0 = p->f0, df = p->df;
  if (!std::isfinite(f0) || !std::isfinite(df) || df == 0) {
    kq_internal_set_error("%s: f0 %g and df %g must be finite and df not 0", fn, f0, df);
    return -1;
  }
  for (int t = 0; t < NT; t += NT - 1)  // the outer two bound the rest
    if (!tc::tone_ok(fn, Fs, f0 + t * df, "tone %d at %g (f0 %g, df %g)", t, f0 + t * df, f0, df)) return -1;
  AlePar np{};
  if (!tc::symbol_period(fn, Fs, b->cfg.block_len, p->baud, "symbol", &np.tb, &np.W)) return -1;
  np.active = 1;
  np.source = p->source;
  for (int t = 0; t < NT; t++) np.inc[t] = (unsigned)std::llrint((f0 + t * df) * 4294967296.0 / Fs);
  b->def.set(slot, np);
  return 0;
}

int kq_ale_remove(kq_ale_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_ale_remove"); }

int kq_ale_process(kq_ale_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_ale_status *status, size_t status_stride) {
  return tc::process<CallArgs>(b, "kq_ale_process", src, format, src_stride, row_stride, block_len, nblocks, on_device, status,
                               status_stride, kWaves, [b](CallArgs &a, unsigned blocks) {
                                 a.golay = b->d.tables.golay;
                                 hipLaunchKernelGGL(k_ale, dim3(blocks), dim3(kThreads), 0, b->stream, a);
                               });
}

int kq_ale_pull_counts(kq_ale_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_ale_pull_counts", counts); }

int kq_ale_pull_event(kq_ale_bank *b, unsigned slot, unsigned index, kq_ale_event *event) {
  return kq::pull_event(b, "kq_ale_pull_event", slot, index, event);
}

int kq_ale_clear_events(kq_ale_bank *b) { return kq::clear_arena(b, "kq_ale_clear_events"); }

int kq_ale_get_table(const kq_ale_bank *b, int16_t *dst, size_t cap) {
  return kq::tonecorr::get_table(b, "kq_ale_get_table", dst, cap);
}

int kq_ale_get_slot(kq_ale_bank *b, unsigned slot, kq_ale_slot *out) {
  std::unique_lock<std::mutex> lk;
  const AlePar *w = tc::wanted(b, "kq_ale_get_slot", slot, out, "out", lk);
  if (!w) return -1;
  for (int t = 0; t < NT; t++) out->inc[t] = w->inc[t];
  out->tb = (uint32_t)w->tb;
  out->W = (uint32_t)w->W;
  return 0;
}

int kq_ale_sync(kq_ale_bank *b) { return kq::sync_bank(b, "kq_ale_sync"); }

int kq_ale_reset(kq_ale_bank *b) { return kq::deferred_reset(b, "kq_ale_reset"); }

}  // extern "C"
