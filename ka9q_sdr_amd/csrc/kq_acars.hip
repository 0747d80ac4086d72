// kq_acars.hip -- ACARS decoder bank: the audio of AM airband channels -> ACARS blocks (2400 bit/s MSK on 1200 / 2400 Hz,
// 7-bit characters with odd parity, CRC-16/KERMIT), as records in per-slot arenas, on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_acars_*): quantise as kq_fsk_*, mix with 1800 Hz from kq_cw_*'s cosine table at a phase
// that is a function of the sample index alone, the matched filter (a half cosine two bits long) at every sample, reduced
// to a; the correlation c of a against the 40 preamble bits one bit apart, its energy e, the threshold and the local
// maximum that make a sync; and, while a block is open, one step per bit: decision against the rotation estimate R, R's
// update, early / late timing, the character, its parity, the CRC and the close.  All exact integers after the quantiser.
// State on the device, per slot: one kq_acars_status record; the past in the form a call needs it -- the last FL - 1
// values of q (two copies, written in turn: a call reads one and writes the other), the last HA values of a and the last
// 2 w of |c|^2 with the threshold's verdict, each a function of the samples alone, so that carrying them changes no
// result -- the open block's bytes and the arena; per bank the table, the taps and the offsets.
//
// k_acars  one wave per slot, `waves` slots to a workgroup (4, or 2 where the history of a high sample rate would not let 4
//          fit 64 KiB of LDS).  A call's samples go through LDS in pieces of `piece` samples (a multiple of 64): every lane mixes samples into Z, then filters its samples of the piece into A behind
//          the HA values of a that the sync looks back on, then correlates: |c|^2 with the threshold's verdict in bit 63
//          goes to C2 behind the 2 w values before the piece.  A lane per sample p = n - w then asks whether p passed and is
//          the maximum of its neighbourhood, and a ballot packs the answers 64 to a word.  Lane 0 walks the piece: with no
//          block open it looks for the next set bit at or behind search_from, else it takes the bits whose sample n has n + w
//          in the piece, reading a at n - e, n and n + e from A.  A and C2 move down by a piece between two pieces.  Every
//          wave of a workgroup has the same pieces, so the barriers are uniform.  The carried record is read once and
//          written once per call.  No atomics, no scratch.
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
using kq::tonecorr::mag;
using kq::tonecorr::sat_inc;
constexpr unsigned kMaxSlots = 4096;
constexpr int kThreads = 256;
constexpr int kPat = 40;                        // preamble bits
constexpr int kMaxTaps = 80;
constexpr int kShift = 30;                      // v -> a
constexpr int kMaxBlockBytes = 256;
constexpr size_t kLdsLimit = 65536;
constexpr unsigned long long kPass = 1ull << 63;
constexpr double kBaud = 2400.0;

struct AcGeom {
  unsigned inc;
  int FL, w, e, tb;
  int H39, HA, H;                // the preamble's reach, values of a in front of a piece, samples a call's results look back on
  int piece, waves;
  unsigned long long dpos;       // bit k: d_k = +1
  unsigned num, den;
  int mpe, mbb, max_blocks;
};

struct AcPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
};

struct CallArgs {
  AcGeom g;
  const AcPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of in.src (host input, staged) or null (par.source)
  const short *table;            // [1024]
  const int *geo;                // [kMaxTaps] hq, [kPat] o_k
  kq_acars_status *state;        // [S]
  const short *hist_r;           // [S][FL - 1]: the q before the call's first sample
  short *hist_w;                 // [S][FL - 1]: the q before the next call's
  int2 *hist_a;                  // [S][HA]: the a before the call's first sample, and then before the next call's
  unsigned long long *hist_c2;   // [S][2 w]: |c|^2 and the verdict, likewise
  unsigned char *open;           // [S][256]
  unsigned char *blocks;         // [S][max_blocks][mbb]
  kq_acars_block_info *info;     // [S][max_blocks]
  unsigned *nblocks;             // [S]
  int nlist;
  int64_t n0, n1;                // the call's samples
  kq::PcmIn in;
  // output
  kq_acars_status *st;
  size_t sstride;
};

// the LDS of a workgroup, in 8-byte words: the table, the taps and offsets, then per wave Z, A, C2 and the flags
__host__ __device__ inline int lds_fixed_words() { return kTable / 2 + kMaxTaps / 2 + kPat / 2; }
__host__ __device__ inline int lds_wave_words(AcGeom const &g) {
  return (g.piece + g.FL - 1) + (g.HA + g.piece) + (2 * g.w + g.piece) + g.piece / 64;
}

// (r + j i) (-j)^m
__device__ __forceinline__ void turn(int r, int i, unsigned m, int &xr, int &xi) {
  m &= 3u;
  xr = m == 0 ? r : m == 1 ? i : m == 2 ? -r : -i;
  xi = m == 0 ? i : m == 1 ? -r : m == 2 ? -i : r;
}

// c and e at the sample whose a is *ap: the header's sums over the 40 preamble bits, OFF[k] = o_k
__device__ __forceinline__ void correlate(const int2 *ap, const int *OFF, unsigned long long dpos, int &cr, int &ci,
                                          unsigned long long &e) {
  cr = ci = 0;
  e = 0;
  for (int k = 0; k < kPat; k++) {
    int2 const a = ap[OFF[k]];
    int xr, xi;
    turn(a.x, a.y, (unsigned)k, xr, xi);
    bool const pos = (dpos >> k) & 1ull;
    cr += pos ? xr : -xr;
    ci += pos ? xi : -xi;
    e += (unsigned long long)((long long)a.x * a.x) + (unsigned long long)((long long)a.y * a.y);
  }
}

struct Out {
  unsigned char *open, *blocks;
  kq_acars_block_info *info;
  unsigned n;
};

// the header's close
__device__ __forceinline__ void close_block(AcGeom const &g, kq_acars_status &s, Out &o, int64_t n, unsigned flags) {
  if (flags & KQ_ACARS_GOOD) s.blocks_good = sat_inc(s.blocks_good);
  else if (flags & KQ_ACARS_OVERRUN) s.overruns = sat_inc(s.overruns);
  else s.blocks_bad = sat_inc(s.blocks_bad);
  if ((flags & KQ_ACARS_GOOD) || s.parity_errors <= (unsigned)g.mpe) {
    if (o.n < (unsigned)g.max_blocks) {
      unsigned char *dst = o.blocks + (size_t)o.n * g.mbb;
      for (unsigned i = 0; i < s.length; i++) dst[i] = o.open[i];
      kq_acars_block_info r;
      r.length = s.length;
      r.flags = flags;
      r.parity_errors = s.parity_errors;
      r.reserved = 0;
      r.sync_sample = s.sync_sample;
      r.end_sample = (uint64_t)n;
      r.sync_c2 = s.sync_c2;
      r.sync_e = s.sync_e;
      r.r2 = (uint64_t)((long long)s.rr * s.rr + (long long)s.ri * s.ri);
      o.info[o.n] = r;
      o.n++;
    } else {
      s.dropped = sat_inc(s.dropped);
    }
  } else {
    s.discarded = sat_inc(s.discarded);
  }
  s.in_block = 0;
  s.ending = 0;
  s.search_from = n + 1;
}

// the header's step of an open block: the bit at sample n; A[0] is a[abase]
__device__ __forceinline__ void take_bit(AcGeom const &g, kq_acars_status &s, Out &o, int64_t n, const int2 *A, int64_t abase) {
  s.t += g.tb;
  s.k++;
  int const at = (int)(n - abase);
  int2 const ac = A[at], ae = A[at - g.e], al = A[at + g.e];
  int ur, ui, er, ei, lr, li;
  turn(ac.x, ac.y, s.k, ur, ui);
  turn(ae.x, ae.y, s.k, er, ei);
  turn(al.x, al.y, s.k, lr, li);
  long long const rr = s.rr, ri = s.ri;
  unsigned const bit = ur * rr + ui * ri >= 0 ? 1u : 0u;
  s.acc += mag(er * rr + ei * ri) - mag(lr * rr + li * ri);
  s.rr += ((bit ? ur : -ur) - s.rr) >> 4;
  s.ri += ((bit ? ui : -ui) - s.ri) >> 4;
  if (++s.cnt == 8) {
    long long const r2 = (long long)s.rr * s.rr + (long long)s.ri * s.ri;
    if (4 * s.acc > r2) s.t -= g.tb >> 5;
    else if (4 * s.acc < -r2) s.t += g.tb >> 5;
    s.acc = 0;
    s.cnt = 0;
  }
  // the frame
  s.cur |= bit << s.nbits;
  s.crc = (s.crc >> 1) ^ (((s.crc ^ bit) & 1u) ? 0x8408u : 0u);
  if (++s.nbits < 8) return;
  unsigned const byte = s.cur;
  s.cur = 0;
  s.nbits = 0;
  if (s.length < (unsigned)kMaxBlockBytes) o.open[s.length] = (unsigned char)byte;  // (mbb <= 256 closes it before)
  s.length++;
  if (s.ending) {  // bytes of the check left, + 4 behind an ETB
    s.ending--;
    if ((s.ending & 3u) == 0) close_block(g, s, o, n, (s.crc == 0 ? KQ_ACARS_GOOD : 0u) | ((s.ending & 4u) ? KQ_ACARS_ETB : 0u));
    return;
  }
  if ((__popc(byte) & 1) == 0) s.parity_errors++;
  unsigned const ch = byte & 0x7fu;
  if ((ch == 0x03u || ch == 0x17u) && s.length + 2 <= (unsigned)g.mbb) s.ending = ch == 0x17u ? 6u : 2u;
  else if (s.length + 2 >= (unsigned)g.mbb) close_block(g, s, o, n, KQ_ACARS_OVERRUN);
}

__global__ __launch_bounds__(kThreads) void k_acars(CallArgs c) {
  extern __shared__ unsigned long long lds[];
  AcGeom const &g = c.g;
  int *CS = reinterpret_cast<int *>(lds);                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  int *HQ = CS + kTable;
  int *OFF = HQ + kMaxTaps;
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * g.waves + wave;
  unsigned long long *mine = lds + lds_fixed_words() + (size_t)wave * lds_wave_words(g);
  int2 *Z = reinterpret_cast<int2 *>(mine);                      // z of [ps - FL + 1, pe)
  int2 *A = Z + (g.piece + g.FL - 1);                            // a of [ps - HA, pe)
  unsigned long long *C2 = mine + (g.piece + g.FL - 1) + (g.HA + g.piece);  // |c|^2 and the verdict, of [ps - 2 w, pe)
  unsigned long long *FLAG = C2 + (2 * g.w + g.piece);           // the syncs among p = ps - w + i, 64 to a word
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  kq::tonecorr::load_packed_table(CS, c.table, tid, (int)blockDim.x);
  for (int i = tid; i < kMaxTaps + kPat; i += (int)blockDim.x) HQ[i] = c.geo[i];  // (OFF lies behind HQ)
  AcPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const FL = g.FL, w = g.w, HA = g.HA, piece = g.piece;
  const short *hr = c.hist_r + (size_t)slot * (FL - 1);
  int2 *ha = c.hist_a + (size_t)slot * HA;
  unsigned long long *hc = c.hist_c2 + (size_t)slot * (2 * w);
  int64_t const n0 = c.n0, n1 = c.n1, q0 = n0 - (FL - 1);      // q0: the sample of hr[0]
  auto getq = [&](int64_t n) -> int { return n < n0 ? (int)hr[n - q0] : kq::load_q(c.in, row, (unsigned)(n - n0)); };
  kq_acars_status s{};
  Out o{};
  if (live && lane == 0) {
    s = c.state[slot];
    o.open = c.open + (size_t)slot * kMaxBlockBytes;
    o.blocks = c.blocks + (size_t)slot * g.max_blocks * g.mbb;
    o.info = c.info + (size_t)slot * g.max_blocks;
    o.n = c.nblocks[slot];
  }
  if (live) {  // the carried a and |c|^2 lie in front of the first piece (the loop's first barrier makes them visible)
    for (int i = lane; i < HA; i += 64) A[i] = ha[i];
    for (int i = lane; i < 2 * w; i += 64) C2[i] = hc[i];
  }
  for (int64_t ps = n0; ps < n1; ps += piece) {
    int64_t const pe = ps + piece < n1 ? ps + piece : n1;
    int const len = (int)(pe - ps);
    __syncthreads();  // the piece before is done with Z and FLAG (and, at the first, the tables are there)
    if (live) {
      int64_t const z0 = ps - (FL - 1);
      for (int i = lane; i < len + FL - 1; i += 64) {
        int64_t const n = z0 + i;
        int const q = getq(n);
        int const cs = CS[((unsigned)n * g.inc) >> 22];        // (n inc) mod 2^32 needs n mod 2^32 only
        Z[i] = make_int2(q * (int)(short)cs, -q * (cs >> 16));
      }
    }
    __syncthreads();
    if (live) {
      for (int i = lane; i < len; i += 64) {                    // v[n] = sum hq[t] z[n - t], n = ps + i
        long long vr = 0, vi = 0;
        const int2 *zp = Z + i + FL - 1;
        for (int t = 0; t < FL; t++) {
          int2 const z = zp[-t];
          int const h = HQ[t];
          vr += (long long)h * z.x;
          vi += (long long)h * z.y;
        }
        A[HA + i] = make_int2((int)(vr >> kShift), (int)(vi >> kShift));
      }
    }
    __syncthreads();
    if (live) {
      for (int i = lane; i < len; i += 64) {                    // c, e, the verdict at n = ps + i
        int cr, ci;
        unsigned long long e;
        correlate(A + HA + i, OFF, g.dpos, cr, ci, e);
        unsigned long long const c2 = (unsigned long long)((long long)cr * cr) + (unsigned long long)((long long)ci * ci);
        C2[2 * w + i] = c2 | (c2 > 0 && c2 * g.den >= e * (kPat * g.num) ? kPass : 0ull);
      }
    }
    __syncthreads();
    for (int i0 = 0; i0 < piece; i0 += 64) {                    // is p = ps - w + i a sync?  (|c|^2 of p is C2[w + i])
      int const i = i0 + lane;
      bool flag = false;
      if (live && i < len) {
        unsigned long long const v = C2[w + i];
        if (v & kPass) {
          unsigned long long const me = v & ~kPass;
          flag = true;
          for (int d = 1; d <= w; d++)
            flag = flag && (C2[w + i - d] & ~kPass) < me && (C2[w + i + d] & ~kPass) <= me;
        }
      }
      unsigned long long const m = __ballot(flag);
      if (lane == 0) FLAG[i0 >> 6] = m;
    }
    __syncthreads();
    int64_t const lo = ps - w, hi = pe - w;                     // the p of this piece
    if (live && lane == 0) {
      int64_t const abase = ps - HA, f0 = ps - w;               // A[0] is a[abase]; bit i of FLAG is p = f0 + i
      for (;;) {
        if (s.in_block) {
          int64_t const nb = (s.t + g.tb + 128) >> 8;
          if (nb >= hi) break;
          take_bit(g, s, o, nb, A, abase);
          continue;
        }
        int64_t const from = s.search_from > lo ? s.search_from : lo;
        int i = (int)(from - f0), found = -1;
        int const end = (int)(hi - f0);
        while (from < hi && i < end) {
          unsigned long long const word = FLAG[i >> 6] >> (i & 63);
          if (word) {
            found = i + __ffsll((long long)word) - 1;
            break;
          }
          i = (i | 63) + 1;
        }
        if (found < 0 || found >= end) break;
        int64_t const p = f0 + found;                           // the header's sync at p
        int cr, ci;
        unsigned long long e;
        correlate(A + (int)(p - abase), OFF, g.dpos, cr, ci, e);
        s.syncs = sat_inc(s.syncs);
        s.in_block = 1;
        s.rr = cr >> 5;
        s.ri = ci >> 5;
        s.t = p * 256;
        s.k = 39;
        s.sync_sample = (uint64_t)p;
        s.sync_c2 = (unsigned long long)((long long)cr * cr) + (unsigned long long)((long long)ci * ci);
        s.sync_e = e;
        s.nbits = s.cur = s.length = s.parity_errors = s.crc = s.ending = s.cnt = 0;
        s.acc = 0;
      }
    }
    if (pe < n1) {  // another piece follows (this one was whole): A and C2 move down by it, a lane's read before its write
      for (int i = lane; i < HA; i += 64) {
        int2 const v = A[i + piece];
        A[i] = v;
      }
      for (int i = lane; i < 2 * w; i += 64) {
        unsigned long long const v = C2[i + piece];
        C2[i] = v;
      }
    }
  }
  if (live) {  // what the next call finds in front: the HA and 2 w values that end with the last piece's `last` samples
    int const last = (int)((n1 - n0) - (n1 - n0 - 1) / piece * piece);
    for (int i = lane; i < HA; i += 64) ha[i] = A[last + i];
    for (int i = lane; i < 2 * w; i += 64) hc[i] = C2[last + i];
    short *hw = c.hist_w + (size_t)slot * (FL - 1);
    for (int j = lane; j < FL - 1; j += 64) hw[j] = (short)getq(n1 - (FL - 1) + j);
  }
  if (live && lane == 0) {
    c.state[slot] = s;
    c.nblocks[slot] = o.n;
    if (c.st) c.st[(size_t)slot * c.sstride] = s;
  }
}

// the integers a sample rate makes (the header's formulas, in double)
void make_geometry(double Fs, AcGeom *g, std::vector<int> *geo) {
  g->inc = (unsigned)std::llrint(1800.0 * 4294967296.0 / Fs);
  g->FL = (int)std::llrint(2.0 * Fs / kBaud);
  g->w = (int)std::ceil(Fs / kBaud);
  g->e = std::max(1, (int)std::llrint(Fs / 9600.0));
  g->tb = (int)std::llrint(256.0 * Fs / kBaud);
  geo->assign(kMaxTaps + kPat, 0);
  for (int i = 0; i < g->FL; i++) (*geo)[i] = (int)std::lrint(32767.0 * std::cos(M_PI * (i - (g->FL - 1) / 2.0) / g->FL));
  for (int k = 0; k < kPat; k++) (*geo)[kMaxTaps + k] = (int)std::llrint((k - 39) * Fs / kBaud);
  g->H39 = -(*geo)[kMaxTaps];
  g->HA = g->H39 + 2 * g->w;
  g->H = g->HA + g->FL - 1;
  static const unsigned char pre[5] = {0x2b, 0x2a, 0x16, 0x16, 0x01};
  g->dpos = 0;
  for (int k = 0; k < kPat; k++) {
    unsigned ch = pre[k >> 3];
    if ((__builtin_popcount(ch) & 1) == 0) ch |= 0x80u;
    if ((ch >> (k & 7)) & 1u) g->dpos |= 1ull << k;
  }
  // the largest piece, with 4 waves before 2, that fits the LDS a workgroup may have without asking
  for (int waves : {4, 2})
    for (int piece : {256, 128, 64}) {
      g->waves = waves;
      g->piece = piece;
      if (((size_t)lds_fixed_words() + (size_t)waves * lds_wave_words(*g)) * 8 <= kLdsLimit) return;
    }
}

}  // namespace

struct kq_acars_bank : kq::HostSide {
  static constexpr bool kDeferred = true;
  kq_acars_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  AcGeom g{};
  std::vector<int> geo;                  // hq and o_k as the kernel reads them
  uint64_t n_cur = 0;
  int turn = 0;                          // the copy of the carried q the next call reads
  kq::DeferredSlots<AcPar> def;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<AcPar> slots;
    short *table = nullptr;
    int *geo = nullptr;
    kq_acars_status *state = nullptr;
    short *hist[2] = {nullptr, nullptr};
    int2 *hist_a = nullptr;
    unsigned long long *hist_c2 = nullptr;
    unsigned char *open = nullptr, *blocks = nullptr;
    kq::EventArena<kq_acars_block_info> arena;
    kq_acars_status *st = nullptr;       // host-memory calls
  } d;

  int to_device();
};

namespace {

int make_device(kq_acars_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots, H = (size_t)b->g.FL - 1;
  if (d.slots.alloc(*b, S) || kq::tonecorr::alloc_table(*b, &d.table) || b->alloc(&d.geo, b->geo.size()) ||
      b->alloc(&d.state, S, true) || b->alloc(&d.hist[0], S * H, true) || b->alloc(&d.hist[1], S * H, true) ||
      b->alloc(&d.hist_a, S * (size_t)b->g.HA, true) || b->alloc(&d.hist_c2, S * 2 * (size_t)b->g.w, true) ||
      b->alloc(&d.open, S * kMaxBlockBytes, true) || b->alloc(&d.blocks, S * b->cfg.max_blocks * b->cfg.max_block_bytes) ||
      d.arena.alloc(*b, S, b->cfg.max_blocks))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.geo, b->geo.data(), b->geo.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // namespace

// kq::DeferredSlots::flush; the record and the carried q, a and |c|^2 of a slot that is set start cold (all zero: the
// header's state at the set) and its arena empty
int kq_acars_bank::to_device() {
  return def.flush(this, make_device, [this](size_t s0, size_t n) {
    KQ_TRY(hipMemsetAsync(d.state + s0, 0, n * sizeof(kq_acars_status), stream));
    size_t const H = (size_t)g.FL - 1;
    for (short *h : d.hist) KQ_TRY(hipMemsetAsync(h + s0 * H, 0, n * H * sizeof(short), stream));
    KQ_TRY(hipMemsetAsync(d.hist_a + s0 * (size_t)g.HA, 0, n * (size_t)g.HA * sizeof(int2), stream));
    KQ_TRY(hipMemsetAsync(d.hist_c2 + s0 * 2 * (size_t)g.w, 0, n * 2 * (size_t)g.w * sizeof(unsigned long long), stream));
    return d.arena.clear(*this, s0, n);
  });
}

extern "C" {

kq_acars_bank *kq_acars_create(const kq_acars_config *cfg) {
  const char *fn = "kq_acars_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  if (!kq::samprate_ok(fn, cfg->samprate)) return nullptr;
  if (cfg->samprate < 4 * kBaud || cfg->samprate > 40 * kBaud) {
    kq_internal_set_error("%s: samprate %.10g must be 9600..96000 (4 to 40 samples per bit of 2400 bit/s)", fn, cfg->samprate);
    return nullptr;
  }
  if (!kq::input_scale_ok(fn, cfg->input_scale) || !kq::field_in_range(fn, "sync_den", cfg->sync_den, 1, 255) ||
      !kq::field_in_range(fn, "sync_num", cfg->sync_num, 1, cfg->sync_den) ||
      !kq::field_in_range(fn, "max_parity_errors", cfg->max_parity_errors, 0, 255) ||
      !kq::field_in_range(fn, "max_block_bytes", cfg->max_block_bytes, 16, kMaxBlockBytes) ||
      !kq::field_in_range(fn, "max_slots", cfg->max_slots, 1, kMaxSlots) ||
      !kq::field_in_range(fn, "max_blocks", cfg->max_blocks, 1, 4096) || !kq::max_samples_ok(fn, cfg->max_samples))
    return nullptr;
  (void)kq::tonecorr::cos_table();  // the table exists from here on
  kq_acars_bank *b = new kq_acars_bank;
  b->cfg = *cfg;
  b->def.init(cfg->max_slots);
  AcGeom &g = b->g;
  make_geometry(cfg->samprate, &g, &b->geo);
  g.num = cfg->sync_num;
  g.den = cfg->sync_den;
  g.mpe = (int)cfg->max_parity_errors;
  g.mbb = (int)cfg->max_block_bytes;
  g.max_blocks = (int)cfg->max_blocks;
  return b;
}

int kq_acars_destroy(kq_acars_bank *b) { return kq::destroy_bank(b, "kq_acars_destroy"); }

int kq_acars_set(kq_acars_bank *b, unsigned slot, const kq_acars_params *p) {
  const char *fn = "kq_acars_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  AcPar np{};
  np.active = 1;
  np.source = p->source;
  b->def.set(slot, np);
  return 0;
}

int kq_acars_remove(kq_acars_bank *b, unsigned slot) { return kq::deferred_remove(b, slot, "kq_acars_remove"); }

int kq_acars_process(kq_acars_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                     unsigned nblocks, int on_device, kq_acars_status *status, size_t status_stride) {
  const char *fn = "kq_acars_process";
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
  AcGeom const &g = b->g;
  size_t const nlist = d.slots.all.size();
  CallArgs a{};
  a.g = g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.table = d.table;
  a.geo = d.geo;
  a.state = d.state;
  a.hist_r = d.hist[b->turn];
  a.hist_w = d.hist[b->turn ^ 1];
  a.hist_a = d.hist_a;
  a.hist_c2 = d.hist_c2;
  a.open = d.open;
  a.blocks = d.blocks;
  a.info = d.arena.ev;
  a.nblocks = d.arena.n;
  a.nlist = (int)nlist;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  if (kq::bind_pcm(&a.in, &a.rowmap, *b, d.slots, b->cfg.max_samples, b->cfg.input_scale, src, format, src_stride, row_stride, block_len,
                   nblocks, on_device) ||
      kq::bind_status(b, on_device, status, status_stride, &a.st, &a.sstride))
    return -1;
  size_t const lds = ((size_t)lds_fixed_words() + (size_t)g.waves * lds_wave_words(g)) * 8;
  hipLaunchKernelGGL(k_acars, dim3((unsigned)((nlist + g.waves - 1) / g.waves)), dim3(64 * g.waves), lds, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->turn ^= 1;  // from here on the carried q is in the other copy, whatever fails below
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_acars_pull_counts(kq_acars_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_acars_pull_counts", counts); }

int kq_acars_pull_block(kq_acars_bank *b, unsigned slot, unsigned index, unsigned char *dst, size_t cap,
                        kq_acars_block_info *info) {
  const char *fn = "kq_acars_pull_block";
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("%s: null dst", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  std::optional<kq::DeviceScope> scope;
  kq_acars_block_info r;
  size_t at;
  if (kq::pull_record(b, fn, slot, index, "blocks", &r, &at, scope)) return -1;
  size_t const take = std::min(cap, (size_t)r.length);
  if (take) {
    KQ_TRY(hipMemcpyAsync(dst, b->d.blocks + at * b->cfg.max_block_bytes, take, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (info) *info = r;
  return (int)r.length;
}

int kq_acars_clear_blocks(kq_acars_bank *b) { return kq::clear_arena(b, "kq_acars_clear_blocks"); }

int kq_acars_get_taps(const kq_acars_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_acars_get_taps: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_acars_get_taps: null dst");
    return -1;
  }
  size_t const n = std::min(cap, (size_t)b->g.FL);
  for (size_t i = 0; i < n; i++) dst[i] = (int16_t)b->geo[i];
  return b->g.FL;
}

int kq_acars_get_slot(kq_acars_bank *b, unsigned slot, kq_acars_slot *out) {
  if (!b) {
    kq_internal_set_error("kq_acars_get_slot: null bank");
    return -1;
  }
  if (!out) {
    kq_internal_set_error("kq_acars_get_slot: null out");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("kq_acars_get_slot: slot %u holds no decoder", slot);
    return -1;
  }
  AcGeom const &g = b->g;
  out->source = b->def.want[slot].source;
  out->inc = g.inc;
  out->taps = (uint32_t)g.FL;
  out->w = (uint32_t)g.w;
  out->e = (uint32_t)g.e;
  out->tb = (uint32_t)g.tb;
  out->history = (uint32_t)g.H;
  out->piece = (uint32_t)g.piece;
  return 0;
}

int kq_acars_sync(kq_acars_bank *b) { return kq::sync_bank(b, "kq_acars_sync"); }

int kq_acars_reset(kq_acars_bank *b) { return kq::deferred_reset(b, "kq_acars_reset"); }

}  // extern "C"
