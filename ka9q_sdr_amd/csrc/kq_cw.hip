// kq_cw.hip -- CW (Morse) decoder bank: the audio of CW channels -> characters, as events (code, elements, dot length,
// start, end, peak) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_cw_*): quantise as kq_tone_*, correlate every frame of B samples against one tone from
// the 1024-entry cosine table with a phase that is a function of the sample index alone, and step the tracker (peak,
// floor, threshold with hysteresis, debounce, dot-length tracking, character and word gaps) once per completed frame.  All
// exact integers after the quantiser.  State on the device, per slot: one kq_cw_status record (the open frame's I and Q
// and the whole tracker) and the arena of events; per bank the table.
//
// k_cw  one wave per slot, four slots to a workgroup.  A slot has one tone and frames of a few dozen samples, so a
//       workgroup per slot (k_tone) would leave most of its lanes without work.  The call's samples go through LDS once, a
//       piece of 64 / L frames at a time, quantised as they are loaded (coalesced: lane i takes samples i, i + 64, ...),
//       each frame at a stride Bs >= B with Bs / 2 odd, so that lanes reading sample i of 32 consecutive frames hit 32
//       banks.  Lane (f, p) of 64 / L x L takes samples p, p + L, ... of frame f against the table (cosine and sine packed
//       in one LDS word), two 64-bit multiply-adds a sample; its phase comes from the sample index.  L = 1 where 64 frames
//       fit the piece and the call has that many: then no lane ever talks to another.  Otherwise the L partial sums of a
//       frame are folded by shuffles; the sums are exact, so L changes no result, and the host picks it per call: the
//       least that fits the piece, and more where the call has too few frames to fill the wave.  The frame leaders
//       square into LDS and lane 0 walks the piece's P values in order through the tracker; the other waves of the
//       workgroup meet it at the next barrier (every wave has the same pieces: the frame grid is shared).  The carried
//       record is read once and written once per call.  No atomics, no scratch.
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

namespace {

constexpr unsigned kMaxSlots = 16384;
constexpr int kTable = 1024;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 4288;                     // samples a wave keeps in LDS: 64 frames of B = 64 at stride 66, and a few more
constexpr unsigned kRunMax = 0x0FFFFFFFu;

struct CwGeom {
  int B, Bs;                     // Bs: a frame's stride in LDS, >= B, Bs / 2 odd
  unsigned magic;                // ceil(2^32 / B): x / B = umulhi(x, magic) for x < 2^16
  unsigned deb, warm, snr, u_min, u_max;
  unsigned long long min_p;
  int max_events;
  float scale;
};

struct CwPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc, u0;
};

struct CallArgs {
  CwGeom g;
  const CwPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of `src` (host input, staged) or null (par.source)
  const short *table;            // [1024]
  kq_cw_status *state;           // [S]
  kq_cw_event *ev;               // [S][max_events]
  unsigned *nev;                 // [S]
  int nlist;
  int L;                         // lanes to a frame, a power of two <= 64
  int64_t n0, n1;                // the call's samples
  // input
  const void *src;
  int format;
  size_t src_stride, row_stride;
  unsigned block_len;
  // output
  kq_cw_status *st;
  size_t sstride;
};

// q of the call's i-th sample (i < 2^28)
__device__ __forceinline__ int load_q(CallArgs const &a, size_t row, unsigned i) {
  unsigned const k = i / a.block_len, j = i - k * a.block_len;
  size_t const idx = row * a.src_stride + (size_t)k * a.row_stride + j;
  if (a.format == KQ_PCM_S16BE) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a.src) + 2 * idx;
    int const w = (int)(short)(unsigned short)(((unsigned)p[0] << 8) | p[1]);
    return w < -32767 ? -32767 : w;
  }
  float const v = rintf(reinterpret_cast<const float *>(a.src)[idx] * a.g.scale);
  if (!(v == v)) return 0;
  return (int)fminf(fmaxf(v, -32767.f), 32767.f);
}

__device__ __forceinline__ void file_event(CwGeom const &g, kq_cw_status &s, unsigned code, unsigned nelem,
                                           unsigned long long start, unsigned long long end, kq_cw_event *ev, unsigned &nev) {
  s.events++;
  if (nev >= (unsigned)g.max_events) {
    s.dropped++;
    return;
  }
  kq_cw_event r;
  r.code = code;
  r.nelem = nelem;
  r.unit = s.unit;
  r.reserved = 0;
  r.start_sample = start * (unsigned long long)g.B;
  r.end_sample = end * (unsigned long long)g.B;
  r.peak = s.hi;
  ev[nev++] = r;
}

// the header's step 6: a mark of `run` frames closes
__device__ __forceinline__ void close_mark(CwGeom const &g, kq_cw_status &s, unsigned run) {
  int const m = (int)(16u * run);  // run < 2^28
  int u = (int)s.unit;             // <= 2^20
  if (m > 8 * u) {
    s.code = 0;
  } else if (m < 2 * u) {
    s.code = 2 * s.code;
    u += (m - u) >> 2;
  } else {
    s.code = 2 * s.code + (s.code ? 1u : 0u);
    u += (m / 3 - u) >> 2;
  }
  s.unit = (unsigned)min(max(u, (int)g.u_min), (int)g.u_max);
  s.nelem++;
  if (s.nelem > 8) s.code = 0;
  s.flags = 0;
}

// the header's tracker: frame k with power P
__device__ __forceinline__ void track(CwGeom const &g, kq_cw_status &s, unsigned long long P, unsigned long long k,
                                      kq_cw_event *ev, unsigned &nev) {
  if (s.frames != 0xFFFFFFFFu) s.frames++;
  if (P > s.hi)
    s.hi = P;
  else
    s.hi -= s.hi >> 8;
  bool const valid = s.frames >= g.warm && s.hi >= g.min_p && s.hi >= (s.lo >> 4) * g.snr;
  unsigned long long const d = s.hi > s.lo ? s.hi - s.lo : 0;
  unsigned long long const thr = s.lo + (s.key ? d >> 3 : d >> 2);
  unsigned const lev = valid && P >= thr ? 1u : 0u;
  if (lev == 0 || (s.key && 16ull * s.run > 8ull * s.unit)) s.lo = (unsigned long long)((long long)s.lo + (((long long)P - (long long)s.lo) >> 5));
  if (lev == s.key) {
    s.run = min(s.run + 1 + s.cand, kRunMax);
    s.cand = 0;
  } else {
    s.cand++;
    if (s.cand >= g.deb) {
      if (s.key) {
        close_mark(g, s, s.run);
        s.last = k + 1 - s.cand;
      } else if (s.nelem == 0) {
        s.first = k + 1 - s.cand;
      }
      s.key = lev;
      s.run = s.cand;
      s.cand = 0;
    }
  }
  if (!s.key) {
    if (!(s.flags & 1) && 16ull * s.run >= 2ull * s.unit) {
      file_event(g, s, s.code, s.nelem, s.first, s.last, ev, nev);
      s.code = 1;
      s.nelem = 0;
      s.flags |= 1;
    }
    if (!(s.flags & 2) && 16ull * s.run >= 5ull * s.unit) {
      file_event(g, s, 1, 0, s.last, k + 1, ev, nev);
      s.flags |= 2;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_cw(CallArgs c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ unsigned long long Pb[kWaves][64];
  __shared__ long long carry[kWaves][2];
  CwGeom const &g = c.g;
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * kWaves + wave;
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  for (int i = tid; i < kTable; i += kThreads)
    CS[i] = ((int)c.table[i] & 0xFFFF) | ((int)c.table[(i - 256) & (kTable - 1)] << 16);
  CwPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const B = g.B, L = c.L, F = 64 / L, f = lane / L, p = lane & (L - 1);
  unsigned const inc = par.inc, step = (unsigned)L * inc;
  // carried: lane 0 holds the record, the open frame's I and Q in it
  kq_cw_status s{};
  unsigned nev = 0;
  kq_cw_event *ev = c.ev + (size_t)slot * g.max_events;
  if (live && lane == 0) {
    s = c.state[slot];
    nev = c.nev[slot];
  }
  long long cI = s.acc_i, cQ = s.acc_q;
  short *q = qs[wave];
  int64_t n = c.n0, k0 = c.n0 / B;
  while (n < c.n1) {  // one piece: the frames k0 .. k0 + F - 1, from n to their end or the call's; x counts from k0 B
    int64_t const pe = (k0 + F) * (int64_t)B, e = pe < c.n1 ? pe : c.n1;
    int const x0 = (int)(n - k0 * B), x1 = x0 + (int)(e - n);  // x1 <= F B
    __syncthreads();  // the piece before is done with q, Pb and carry (and the first finds CS loaded)
    if (live) {
      for (int x = x0 + lane; x < x1; x += 64) {
        unsigned const fr = __umulhi((unsigned)x, g.magic);
        q[fr * g.Bs + ((unsigned)x - fr * (unsigned)B)] = (short)load_q(c, row, (unsigned)(n - c.n0) + (unsigned)(x - x0));
      }
    }
    __syncthreads();
    long long sI = 0, sQ = 0;
    int const xa = x0 > f * B ? x0 : f * B, xb = x1 < (f + 1) * B ? x1 : (f + 1) * B;
    if (live) {
      unsigned ph = ((unsigned)(k0 * B) + (unsigned)(xa + p)) * inc;  // (n inc) mod 2^32 needs n mod 2^32 only
      const short *qf = q + f * (g.Bs - B);
      for (int x = xa + p; x < xb; x += L, ph += step) {
        int const v = qf[x], cs = CS[ph >> 22];
        sI += (long long)v * (short)cs;
        sQ += (long long)v * (cs >> 16);
      }
    }
    for (int off = L >> 1; off; off >>= 1) {
      sI += __shfl_xor(sI, off);
      sQ += __shfl_xor(sQ, off);
    }
    if (lane == 0) {  // frame 0 of the call's first piece goes on from the carried sums
      sI += cI;
      sQ += cQ;
      cI = cQ = 0;
    }
    int const done = (int)__umulhi((unsigned)x1, g.magic);  // frames of the piece that are complete
    if (p == 0 && f * B < x1) {
      if (f < done) {
        long long const a = sI >> 15, b = sQ >> 15;
        Pb[wave][f] = (unsigned long long)(a * a) + (unsigned long long)(b * b);
      } else {  // the call ends inside frame f
        carry[wave][0] = sI;
        carry[wave][1] = sQ;
      }
    }
    __syncthreads();
    if (live && lane == 0) {
      for (int i = 0; i < done; i++) track(g, s, Pb[wave][i], (unsigned long long)(k0 + i), ev, nev);
      if (done * B < x1) {
        cI = carry[wave][0];
        cQ = carry[wave][1];
      }
    }
    n = e;
    k0 += F;
  }
  if (live && lane == 0) {
    s.acc_i = cI;
    s.acc_q = cQ;
    c.state[slot] = s;
    c.nev[slot] = nev;
    if (c.st) c.st[(size_t)slot * c.sstride] = s;
  }
}

// C[j] = rint(32767 cos(2 pi j / 1024)), made once
std::vector<short> const &cos_table() {
  static std::vector<short> const table = [] {
    std::vector<short> t((size_t)kTable);
    for (int j = 0; j < kTable; j++) t[j] = (short)std::lrint(32767.0 * std::cos(2.0 * M_PI * j / kTable));
    return t;
  }();
  return table;
}

// the dot of `wpm` in sixteenths of a frame
double unit_of(double Fs, unsigned B, float wpm) { return 19.2 * Fs / ((double)B * (double)wpm); }

}  // namespace

struct kq_cw_bank : kq::HostSide {
  kq_cw_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  CwGeom g{};
  int Lmin = 1;                  // the least lanes to a frame whose piece fits kTile
  uint64_t n_cur = 0;
  // kq_cw_set and kq_cw_remove touch no device: they change `want`, and the next call that needs the device brings the
  // slots in `dirty` there (a cold start for each that is set)
  std::vector<CwPar> want;
  std::vector<unsigned> dirty;
  std::vector<char> is_dirty;
  size_t nwant = 0;              // active entries of `want`
  struct Dev {  // kq::lazy_device
    kq::SlotTable<CwPar> slots;
    short *table = nullptr;
    kq_cw_status *state = nullptr;
    kq_cw_event *ev = nullptr;
    unsigned *nev = nullptr;
    kq_cw_status *st = nullptr;          // host-memory calls
  } d;

  // no device yet and no slot that wants one: the entry points then ask for none
  bool deviceless() const { return !dev_ready && nwant == 0; }

  void touch(unsigned slot) {
    if (is_dirty[slot]) return;
    is_dirty[slot] = 1;
    dirty.push_back(slot);
  }
};

namespace {

int make_device(kq_cw_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots;
  if (d.slots.alloc(*b, S) || b->alloc(&d.table, (size_t)kTable) || b->alloc(&d.state, S, true) ||
      b->alloc(&d.ev, S * (size_t)b->g.max_events) || b->alloc(&d.nev, S, true))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.table, cos_table().data(), kTable * sizeof(short), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// The slots that were set or removed since the last call, to the device: the record of a slot that is set starts cold
// (the header's state at the set) and its arena empty.  Waits for the stream first and last.  Without a device and
// without a slot that wants one nothing happens.
int flush(kq_cw_bank *b) {
  if (b->dirty.empty()) return 0;
  auto forget = [b] {
    for (unsigned s : b->dirty) b->is_dirty[s] = 0;
    b->dirty.clear();
  };
  if (b->deviceless()) {
    forget();
    return 0;
  }
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  auto &t = b->d.slots;
  std::vector<kq_cw_status> cold(b->dirty.size());  // lives until upload() has waited
  for (size_t i = 0; i < b->dirty.size(); i++) {
    unsigned const s = b->dirty[i];
    t.par[s] = b->want[s];
    if (t.par[s].active) {
      kq_cw_status &r = cold[i];
      std::memset(&r, 0, sizeof r);
      r.unit = t.par[s].u0;
      r.code = 1;
      r.flags = 3;
      KQ_TRY(hipMemcpyAsync(b->d.state + s, &r, sizeof r, hipMemcpyHostToDevice, b->stream));
      KQ_TRY(hipMemsetAsync(b->d.nev + s, 0, sizeof(unsigned), b->stream));
    }
    if (i + 1 < b->dirty.size())
      KQ_TRY(hipMemcpyAsync(t.d_par + s, &t.par[s], sizeof(CwPar), hipMemcpyHostToDevice, b->stream));
  }
  if (t.upload(*b, b->dirty.back())) return -1;  // the last record, the active list, and the wait
  forget();
  return 0;
}

bool in_range(unsigned v, unsigned lo, unsigned hi) { return v >= lo && v <= hi; }

}  // namespace

extern "C" {

kq_cw_bank *kq_cw_create(const kq_cw_config *cfg) {
  const char *fn = "kq_cw_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  double const Fs = cfg->samprate;
  if (!(Fs > 0) || !std::isfinite(Fs)) {
    kq_internal_set_error("%s: samprate %.10g must be positive and finite", fn, Fs);
    return nullptr;
  }
  if (!in_range(cfg->block_len, 8, 4096)) {
    kq_internal_set_error("%s: block_len %u must be 8..4096", fn, cfg->block_len);
    return nullptr;
  }
  if (!(cfg->min_wpm > 0) || !std::isfinite(cfg->max_wpm) || !(cfg->min_wpm <= cfg->max_wpm)) {
    kq_internal_set_error("%s: speeds %g..%g WPM must be positive, finite and in order", fn, (double)cfg->min_wpm,
                          (double)cfg->max_wpm);
    return nullptr;
  }
  double const lo = std::floor(unit_of(Fs, cfg->block_len, cfg->max_wpm)), hi = std::ceil(unit_of(Fs, cfg->block_len, cfg->min_wpm));
  if (!(lo >= 48.0)) {
    kq_internal_set_error("%s: max_wpm %g leaves a dot %g sixteenths of a frame of %u samples, fewer than 48 (3 frames)", fn,
                          (double)cfg->max_wpm, lo, cfg->block_len);
    return nullptr;
  }
  if (!(hi <= 1048576.0)) {
    kq_internal_set_error("%s: min_wpm %g makes a dot %g sixteenths of a frame of %u samples, more than 2^20", fn,
                          (double)cfg->min_wpm, hi, cfg->block_len);
    return nullptr;
  }
  if (!in_range(cfg->deb, 1, 16)) {
    kq_internal_set_error("%s: deb %u must be 1..16", fn, cfg->deb);
    return nullptr;
  }
  if (cfg->warm > 65535) {
    kq_internal_set_error("%s: warm %u must be 0..65535", fn, cfg->warm);
    return nullptr;
  }
  if (!in_range(cfg->snr, 16, 4095)) {
    kq_internal_set_error("%s: snr %u must be 16..4095", fn, cfg->snr);
    return nullptr;
  }
  if (cfg->min_p > (1ull << 55)) {
    kq_internal_set_error("%s: min_p %llu must be 0..2^55", fn, (unsigned long long)cfg->min_p);
    return nullptr;
  }
  if (!std::isfinite(cfg->input_scale) || !(cfg->input_scale > 0)) {
    kq_internal_set_error("%s: input_scale must be finite and positive", fn);
    return nullptr;
  }
  if (!in_range(cfg->max_slots, 1, kMaxSlots)) {
    kq_internal_set_error("%s: max_slots %u must be 1..%u", fn, cfg->max_slots, kMaxSlots);
    return nullptr;
  }
  if (!in_range(cfg->max_events, 1, 4096)) {
    kq_internal_set_error("%s: max_events %u must be 1..4096", fn, cfg->max_events);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("%s: max_samples %zu must be 1..2^28", fn, cfg->max_samples);
    return nullptr;
  }
  (void)cos_table();  // the table exists from here on
  kq_cw_bank *b = new kq_cw_bank;
  b->cfg = *cfg;
  b->want.assign(cfg->max_slots, CwPar{});
  b->is_dirty.assign(cfg->max_slots, 0);
  CwGeom &g = b->g;
  g.B = (int)cfg->block_len;
  g.Bs = g.B + ((g.B & 1) ? 1 : 0);  // even
  if ((g.Bs & 3) == 0) g.Bs += 2;    // and Bs / 2 odd
  g.magic = (unsigned)((0x100000000ull + cfg->block_len - 1) / cfg->block_len);
  g.deb = cfg->deb;
  g.warm = cfg->warm;
  g.snr = cfg->snr;
  g.u_min = (unsigned)lo;
  g.u_max = (unsigned)hi;
  g.min_p = cfg->min_p;
  g.max_events = (int)cfg->max_events;
  g.scale = cfg->input_scale;
  while ((64 / b->Lmin) * g.Bs > kTile) b->Lmin *= 2;  // ends at 64 at the latest: Bs <= 4098
  return b;
}

int kq_cw_destroy(kq_cw_bank *b) { return kq::destroy_bank(b, "kq_cw_destroy"); }

int kq_cw_set(kq_cw_bank *b, unsigned slot, const kq_cw_params *p) {
  const char *fn = "kq_cw_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  double const Fs = b->cfg.samprate, f = p->pitch;
  if (!(f > 0) || !(f < 0.5 * Fs)) {
    kq_internal_set_error("%s: pitch %g must be above 0 and below samprate / 2", fn, f);
    return -1;
  }
  if (!(p->wpm >= b->cfg.min_wpm) || !(p->wpm <= b->cfg.max_wpm)) {
    kq_internal_set_error("%s: wpm %g must be within the bank's %g..%g", fn, (double)p->wpm, (double)b->cfg.min_wpm,
                          (double)b->cfg.max_wpm);
    return -1;
  }
  CwPar np{};
  np.active = 1;
  np.source = p->source;
  np.inc = (unsigned)std::llrint(f * 4294967296.0 / Fs);
  np.u0 = std::min(std::max((unsigned)std::llrint(unit_of(Fs, b->cfg.block_len, p->wpm)), b->g.u_min), b->g.u_max);
  b->nwant += !b->want[slot].active;
  b->want[slot] = np;
  b->touch(slot);
  return 0;
}

int kq_cw_remove(kq_cw_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_cw_remove: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots || !b->want[slot].active) {
    kq_internal_set_error("kq_cw_remove: slot %u holds no decoder", slot);
    return -1;
  }
  b->want[slot] = CwPar{};
  b->nwant--;
  b->touch(slot);
  return 0;
}

int kq_cw_process(kq_cw_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                  unsigned nblocks, int on_device, kq_cw_status *status, size_t status_stride) {
  if (!b) {
    kq_internal_set_error("kq_cw_process: null bank");
    return -1;
  }
  if (format != KQ_PCM_F32 && format != KQ_PCM_S16BE) {
    kq_internal_set_error("kq_cw_process: unknown sample format %d", format);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_cw_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  if (status && status_stride < 1) {
    kq_internal_set_error("kq_cw_process: status_stride %zu < 1", status_stride);
    return -1;
  }
  if (ncall == 0) return 0;
  if (!src) {
    kq_internal_set_error("kq_cw_process: null src");
    return -1;
  }
  if (b->deviceless()) {
    (void)flush(b);
    b->n_cur += ncall;
    return 0;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (flush(b)) return -1;
  kq::CallWork const work = kq::call_work(b, "kq_cw_process", ncall, src, "src");
  if (work == kq::CALL_IDLE) {
    b->n_cur += ncall;
    return 0;
  }
  if (work != kq::CALL_RUN) return work;
  auto &d = b->d;
  size_t const S = b->cfg.max_slots, nlist = d.slots.all.size();
  CallArgs a{};
  a.g = b->g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.table = d.table;
  a.state = d.state;
  a.ev = d.ev;
  a.nev = d.nev;
  a.nlist = (int)nlist;
  a.n0 = (int64_t)b->n_cur;
  a.n1 = a.n0 + (int64_t)ncall;
  // lanes to a frame: what the piece needs, and more where the call's frames (at most nf) do not fill a wave
  size_t const nf = (ncall + (size_t)b->g.B - 2) / (size_t)b->g.B + 1;
  a.L = b->Lmin;
  while (a.L < 64 && (size_t)(2 * a.L) * nf <= 64) a.L *= 2;
  a.format = format;
  a.block_len = block_len;
  if (on_device) {
    a.src = src;
    a.src_stride = src_stride;
    a.row_stride = row_stride;
    a.rowmap = nullptr;
    a.st = status;
    a.sstride = status_stride;
  } else {
    kq::Staged in;
    if (d.slots.stage_rows(*b, src, format == KQ_PCM_S16BE ? 2 : 4, src_stride, row_stride, block_len, nblocks,
                           b->cfg.max_samples * 4, &in))
      return -1;
    a.src = in.src;
    a.src_stride = in.src_stride;
    a.row_stride = in.row_stride;
    a.rowmap = in.rowmap;
    if (status && !d.st && b->alloc(&d.st, S)) return -1;
    a.st = status ? d.st : nullptr;
    a.sstride = 1;
  }
  hipLaunchKernelGGL(k_cw, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  if (!on_device) {
    auto back = [&](size_t s0, size_t n) {  // the records of the active slots
      return kq::copy_rows_back(*b, status, status_stride, d.st, 1, 1, sizeof(kq_cw_status), s0, n);
    };
    if (status && d.slots.for_runs(back)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  return 0;
}

int kq_cw_pull_counts(kq_cw_bank *b, uint32_t *counts) {
  if (!b) {
    kq_internal_set_error("kq_cw_pull_counts: null bank");
    return -1;
  }
  if (!counts) {
    kq_internal_set_error("kq_cw_pull_counts: null counts");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (b->deviceless()) {
    (void)flush(b);
    std::memset(counts, 0, b->cfg.max_slots * sizeof(uint32_t));
    return 0;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (flush(b)) return -1;  // a slot set since the last call shows its empty arena
  KQ_TRY(hipMemcpyAsync(counts, b->d.nev, b->cfg.max_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_cw_pull_event(kq_cw_bank *b, unsigned slot, unsigned index, kq_cw_event *event) {
  if (!b) {
    kq_internal_set_error("kq_cw_pull_event: null bank");
    return -1;
  }
  if (!event) {
    kq_internal_set_error("kq_cw_pull_event: null event");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots) {
    kq_internal_set_error("kq_cw_pull_event: slot %u >= max_slots %u", slot, b->cfg.max_slots);
    return -1;
  }
  unsigned n = 0;
  if (b->deviceless()) {
    (void)flush(b);
    kq_internal_set_error("kq_cw_pull_event: slot %u has %u events", slot, n);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (flush(b)) return -1;
  KQ_TRY(hipMemcpyAsync(&n, b->d.nev + slot, sizeof n, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  if (index >= n) {
    kq_internal_set_error("kq_cw_pull_event: slot %u has %u events", slot, n);
    return -1;
  }
  size_t const at = (size_t)slot * b->cfg.max_events + index;
  KQ_TRY(hipMemcpyAsync(event, b->d.ev + at, sizeof *event, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_cw_clear_events(kq_cw_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_cw_clear_events: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipMemsetAsync(b->d.nev, 0, b->cfg.max_slots * sizeof(unsigned), b->stream));
  return 0;
}

int kq_cw_get_table(const kq_cw_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_cw_get_table: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_cw_get_table: null dst");
    return -1;
  }
  size_t const n = std::min(cap, (size_t)kTable);
  if (n) std::memcpy(dst, cos_table().data(), n * sizeof(int16_t));
  return kTable;
}

int kq_cw_get_inc(kq_cw_bank *b, unsigned slot, uint32_t *inc) {
  if (!b) {
    kq_internal_set_error("kq_cw_get_inc: null bank");
    return -1;
  }
  if (!inc) {
    kq_internal_set_error("kq_cw_get_inc: null inc");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots || !b->want[slot].active) {
    kq_internal_set_error("kq_cw_get_inc: slot %u holds no decoder", slot);
    return -1;
  }
  *inc = b->want[slot].inc;
  return 0;
}

int kq_cw_sync(kq_cw_bank *b) { return kq::sync_bank(b, "kq_cw_sync"); }

int kq_cw_reset(kq_cw_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_cw_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  for (unsigned s = 0; s < b->cfg.max_slots; s++)  // every slot that is set starts cold at the next call
    if (b->want[s].active) b->touch(s);
  return 0;
}

}  // extern "C"
