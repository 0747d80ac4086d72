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
// k_rtty  k_cw's mapping: one wave per slot, four slots to a workgroup.  The call's samples go through LDS once, a piece of
//         64 / L frames at a time, quantised as they are loaded, each frame at a stride Bs >= B with Bs / 2 odd.  Lane
//         (f, p) of 64 / L x L takes samples p, p + L, ... of frame f and uses each for both tones: one sample read, two
//         packed table reads, four 64-bit multiply-adds.  The L partial sums of a frame are folded by shuffles; the sums
//         are exact, so L changes no result and the host picks it per call.  The frame leaders write the four reduced
//         sums to LDS behind the 31 carried frames of history (W <= 32), lane f then sums its own W entries per tone and
//         squares -- exact, so no scan order matters -- and lane 0 walks the piece's (Pm, Ps) pairs in order through the
//         levels and the framer.  The baud rate and W differ from slot to slot; B and the frame grid do not, so every wave
//         of a workgroup has the same pieces and the barriers are uniform.  The carried record and the history are read
//         once and written once per call.  No atomics, no scratch.
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
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50; with the rest
                                                // the workgroup stays under 40 KiB, four workgroups to a CU
constexpr int kHist = 31;                       // frames of history a slot carries: W - 1 at the most
constexpr int kRow = kHist + 64 + 1;            // a wave's reduced sums of one kind: the history and a piece's frames
constexpr unsigned kWait = 0, kIdle = 1, kChar = 2;

struct RttyGeom {
  int B, Bs;                     // Bs: a frame's stride in LDS, >= B, Bs / 2 odd
  unsigned magic;                // ceil(2^32 / B): x / B = umulhi(x, magic) for x < 2^16
  unsigned warm, snr;
  unsigned long long min_p;
  int max_events;
  float scale;
};

struct RttyPar {  // per slot, written by the host when a call finds the slot set anew
  int active;
  unsigned source;
  unsigned inc_m, inc_s;
  int tb, W, nbits;
};

struct RttyHist {
  int v[4][kHist];               // a, b of mark, a, b of space; [kHist - 1] is the last completed frame
};

struct CallArgs {
  RttyGeom g;
  const RttyPar *par;
  const int *list;               // active slots, ascending
  const int *rowmap;             // per list entry: the row of `src` (host input, staged) or null (par.source)
  const short *table;            // [1024]
  kq_rtty_status *state;         // [S]
  RttyHist *hist;                // [S]
  kq_rtty_event *ev;             // [S][max_events]
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
  kq_rtty_status *st;
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

__device__ __forceinline__ unsigned sat_inc(unsigned v) { return v == 0xFFFFFFFFu ? v : v + 1; }

__device__ __forceinline__ void file_event(RttyGeom const &g, kq_rtty_status &s, unsigned flags, kq_rtty_event *ev, unsigned &nev) {
  s.events = sat_inc(s.events);
  if (nev >= (unsigned)g.max_events) {
    s.dropped = sat_inc(s.dropped);
    return;
  }
  kq_rtty_event r;
  r.code = s.code;
  r.flags = flags;
  r.start_sample = s.start * (unsigned long long)g.B;
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
  if (s.state != kChar || samp) {  // every value is below 2^63: the differences fit
    int const sh = samp ? 4 : 6;
    s.sig = (unsigned long long)((long long)s.sig + (((long long)hi - (long long)s.sig) >> sh));
    s.nse = (unsigned long long)((long long)s.nse + (((long long)lo - (long long)s.nse) >> sh));
  }
  // 16 sig >= nse snr in 128 bits: (sig >> 60, sig << 4) against (umulhi(nse, snr), nse snr)
  unsigned long long const lh = s.sig >> 60, ll = s.sig << 4, rh = __umul64hi(s.nse, (unsigned long long)g.snr),
                           rl = s.nse * (unsigned long long)g.snr;
  bool const ratio = lh > rh || (lh == rh && ll >= rl);
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
  int const tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = (int)blockIdx.x * kWaves + wave;
  bool const live = li < c.nlist;
  int const slot = live ? c.list[li] : 0;
  for (int i = tid; i < kTable; i += kThreads)
    CS[i] = ((int)c.table[i] & 0xFFFF) | ((int)c.table[(i - 256) & (kTable - 1)] << 16);
  RttyPar const par = c.par[slot];
  size_t const row = live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)par.source;
  int const B = g.B, L = c.L, F = 64 / L, f = lane / L, p = lane & (L - 1);
  int const W = live ? min(max(par.W, 1), kHist + 1) : 1;  // (the host keeps it in 8..32)
  unsigned const inc_m = par.inc_m, inc_s = par.inc_s, step_m = (unsigned)L * inc_m, step_s = (unsigned)L * inc_s;
  // carried: lane 0 holds the record, the open frame's sums in it; the history goes to the front of A
  kq_rtty_status s{};
  unsigned nev = 0;
  kq_rtty_event *ev = c.ev + (size_t)slot * g.max_events;
  if (live && lane == 0) {
    s = c.state[slot];
    nev = c.nev[slot];
  }
  if (lane < kHist)
    for (int t = 0; t < 4; t++) A[wave][t][lane] = live ? c.hist[slot].v[t][lane] : 0;
  long long cy[4] = {s.acc_im, s.acc_qm, s.acc_is, s.acc_qs};
  short *q = qs[wave];
  int64_t n = c.n0, k0 = c.n0 / B;
  while (n < c.n1) {  // one piece: the frames k0 .. k0 + F - 1, from n to their end or the call's; x counts from k0 B
    int64_t const pe = (k0 + F) * (int64_t)B, e = pe < c.n1 ? pe : c.n1;
    int const x0 = (int)(n - k0 * B), x1 = x0 + (int)(e - n);  // x1 <= F B
    __syncthreads();  // the piece before is done with q, A, Pb, carry and lastsum (and the first finds CS and A loaded)
    if (live) {
      for (int x = x0 + lane; x < x1; x += 64) {
        unsigned const fr = __umulhi((unsigned)x, g.magic);
        q[fr * g.Bs + ((unsigned)x - fr * (unsigned)B)] = (short)load_q(c, row, (unsigned)(n - c.n0) + (unsigned)(x - x0));
      }
    }
    __syncthreads();
    long long sm[4] = {0, 0, 0, 0};
    int const xa = x0 > f * B ? x0 : f * B, xb = x1 < (f + 1) * B ? x1 : (f + 1) * B;
    if (live) {
      unsigned const at = (unsigned)(k0 * B) + (unsigned)(xa + p);  // (n inc) mod 2^32 needs n mod 2^32 only
      unsigned pm = at * inc_m, ps = at * inc_s;
      const short *qf = q + f * (g.Bs - B);
      for (int x = xa + p; x < xb; x += L, pm += step_m, ps += step_s) {
        int const v = qf[x], cm = CS[pm >> 22], cs = CS[ps >> 22];
        sm[0] += (long long)v * (short)cm;
        sm[1] += (long long)v * (cm >> 16);
        sm[2] += (long long)v * (short)cs;
        sm[3] += (long long)v * (cs >> 16);
      }
    }
    for (int off = L >> 1; off; off >>= 1)
      for (int t = 0; t < 4; t++) sm[t] += __shfl_xor(sm[t], off);
    if (lane == 0)  // frame 0 of the call's first piece goes on from the carried sums
      for (int t = 0; t < 4; t++) {
        sm[t] += cy[t];
        cy[t] = 0;
      }
    int const done = (int)__umulhi((unsigned)x1, g.magic);  // frames of the piece that are complete
    if (p == 0 && f * B < x1) {
      if (f < done) {
        for (int t = 0; t < 4; t++) A[wave][t][kHist + f] = (int)(sm[t] >> 12);
      } else {  // the call ends inside frame f
        for (int t = 0; t < 4; t++) carry[wave][t] = sm[t];
      }
    }
    __syncthreads();
    int keep[4] = {0, 0, 0, 0};
    if (lane < done) {  // the window that ends at frame `lane` of the piece: W entries, the last at kHist + lane
      int w[4] = {0, 0, 0, 0};
      for (int i = 0; i < W; i++)
        for (int t = 0; t < 4; t++) w[t] += A[wave][t][kHist + lane - i];
      Pb[wave][0][lane] = (unsigned long long)((long long)w[0] * w[0]) + (unsigned long long)((long long)w[1] * w[1]);
      Pb[wave][1][lane] = (unsigned long long)((long long)w[2] * w[2]) + (unsigned long long)((long long)w[3] * w[3]);
      if (lane == done - 1)
        for (int t = 0; t < 4; t++) lastsum[wave][t] = w[t];
    }
    if (lane < kHist)  // what the next piece finds in front: the last kHist frames
      for (int t = 0; t < 4; t++) keep[t] = A[wave][t][done + lane];
    __syncthreads();
    if (lane < kHist)
      for (int t = 0; t < 4; t++) A[wave][t][lane] = keep[t];
    if (live && lane == 0) {
      for (int i = 0; i < done; i++) step(g, par, s, Pb[wave][0][i], Pb[wave][1][i], (unsigned long long)(k0 + i), ev, nev);
      if (done) {
        s.sum_im = lastsum[wave][0];
        s.sum_qm = lastsum[wave][1];
        s.sum_is = lastsum[wave][2];
        s.sum_qs = lastsum[wave][3];
      }
      if (done * B < x1)
        for (int t = 0; t < 4; t++) cy[t] = carry[wave][t];
    }
    n = e;
    k0 += F;
  }
  __syncthreads();
  if (live && lane < kHist)
    for (int t = 0; t < 4; t++) c.hist[slot].v[t][lane] = A[wave][t][lane];
  if (live && lane == 0) {
    s.acc_im = cy[0];
    s.acc_qm = cy[1];
    s.acc_is = cy[2];
    s.acc_qs = cy[3];
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

}  // namespace

struct kq_rtty_bank : kq::HostSide {
  kq_rtty_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  RttyGeom g{};
  int Lmin = 1;                  // the least lanes to a frame whose piece fits kTile
  uint64_t n_cur = 0;
  // kq_rtty_set and kq_rtty_remove touch no device: they change `want`, and the next call that needs the device brings
  // the slots in `dirty` there (a cold start for each that is set)
  std::vector<RttyPar> want;
  std::vector<unsigned> dirty;
  std::vector<char> is_dirty;
  size_t nwant = 0;              // active entries of `want`
  struct Dev {  // kq::lazy_device
    kq::SlotTable<RttyPar> slots;
    short *table = nullptr;
    kq_rtty_status *state = nullptr;
    RttyHist *hist = nullptr;
    kq_rtty_event *ev = nullptr;
    unsigned *nev = nullptr;
    kq_rtty_status *st = nullptr;        // host-memory calls
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

int make_device(kq_rtty_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots;
  if (d.slots.alloc(*b, S) || b->alloc(&d.table, (size_t)kTable) || b->alloc(&d.state, S, true) || b->alloc(&d.hist, S, true) ||
      b->alloc(&d.ev, S * (size_t)b->g.max_events) || b->alloc(&d.nev, S, true))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.table, cos_table().data(), kTable * sizeof(short), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// The slots that were set or removed since the last call, to the device: the record and the history of a slot that is set
// start cold (all zero: the header's state at the set) and its arena empty.  Consecutive slots go together: a run of them
// costs one copy of its parameters and, where they are set, three memsets, however long it is (4096 slots set before the
// first call are four runtime calls, not sixteen thousand).  Waits for the stream first and last.  Without a device and
// without a slot that wants one nothing happens.
int flush(kq_rtty_bank *b) {
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
  std::sort(b->dirty.begin(), b->dirty.end());
  for (unsigned s : b->dirty) t.par[s] = b->want[s];
  for (size_t i = 0; i < b->dirty.size();) {  // a run: consecutive slots, all set or all removed
    unsigned const s0 = b->dirty[i];
    int const set = t.par[s0].active;
    size_t j = i + 1;
    while (j < b->dirty.size() && b->dirty[j] == b->dirty[j - 1] + 1 && t.par[b->dirty[j]].active == set) j++;
    size_t const n = j - i;
    if (set) {
      KQ_TRY(hipMemsetAsync(b->d.state + s0, 0, n * sizeof(kq_rtty_status), b->stream));
      KQ_TRY(hipMemsetAsync(b->d.hist + s0, 0, n * sizeof(RttyHist), b->stream));
      KQ_TRY(hipMemsetAsync(b->d.nev + s0, 0, n * sizeof(unsigned), b->stream));
    }
    KQ_TRY(hipMemcpyAsync(t.d_par + s0, &t.par[s0], n * sizeof(RttyPar), hipMemcpyHostToDevice, b->stream));  // (t.par stays)
    i = j;
  }
  if (t.upload(*b, b->dirty.back())) return -1;  // the active list and the wait (and that one record once more)
  forget();
  return 0;
}

bool in_range(unsigned v, unsigned lo, unsigned hi) { return v >= lo && v <= hi; }

}  // namespace

extern "C" {

kq_rtty_bank *kq_rtty_create(const kq_rtty_config *cfg) {
  const char *fn = "kq_rtty_create";
  if (!cfg) {
    kq_internal_set_error("%s: null config", fn);
    return nullptr;
  }
  double const Fs = cfg->samprate;
  if (!(Fs > 0) || !std::isfinite(Fs)) {
    kq_internal_set_error("%s: samprate %.10g must be positive and finite", fn, Fs);
    return nullptr;
  }
  if (!in_range(cfg->block_len, 8, 256)) {
    kq_internal_set_error("%s: block_len %u must be 8..256", fn, cfg->block_len);
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
  kq_rtty_bank *b = new kq_rtty_bank;
  b->cfg = *cfg;
  b->want.assign(cfg->max_slots, RttyPar{});
  b->is_dirty.assign(cfg->max_slots, 0);
  RttyGeom &g = b->g;
  g.B = (int)cfg->block_len;
  g.Bs = g.B + ((g.B & 1) ? 1 : 0);  // even
  if ((g.Bs & 3) == 0) g.Bs += 2;    // and Bs / 2 odd
  g.magic = (unsigned)((0x100000000ull + cfg->block_len - 1) / cfg->block_len);
  g.warm = cfg->warm;
  g.snr = cfg->snr;
  g.min_p = cfg->min_p;
  g.max_events = (int)cfg->max_events;
  g.scale = cfg->input_scale;
  while ((64 / b->Lmin) * g.Bs > kTile) b->Lmin *= 2;  // ends at 8: Bs <= 258
  return b;
}

int kq_rtty_destroy(kq_rtty_bank *b) { return kq::destroy_bank(b, "kq_rtty_destroy"); }

int kq_rtty_set(kq_rtty_bank *b, unsigned slot, const kq_rtty_params *p) {
  const char *fn = "kq_rtty_set";
  if (!kq::set_args_ok(fn, slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank(fn, slot, b->cfg.max_slots)) return -1;
  double const Fs = b->cfg.samprate, fm = p->mark, fs = p->space, baud = p->baud;
  if (!(fm > 0) || !(fm < 0.5 * Fs)) {
    kq_internal_set_error("%s: mark %g must be above 0 and below samprate / 2", fn, fm);
    return -1;
  }
  if (!(fs > 0) || !(fs < 0.5 * Fs)) {
    kq_internal_set_error("%s: space %g must be above 0 and below samprate / 2", fn, fs);
    return -1;
  }
  if (p->mark == p->space) {
    kq_internal_set_error("%s: mark and space are both %g", fn, fm);
    return -1;
  }
  if (!in_range(p->nbits, 5, 8)) {
    kq_internal_set_error("%s: nbits %u must be 5..8", fn, p->nbits);
    return -1;
  }
  if (!(baud > 0) || !std::isfinite(baud)) {
    kq_internal_set_error("%s: baud %g must be positive and finite", fn, baud);
    return -1;
  }
  double const tb = std::rint(256.0 * Fs / ((double)b->cfg.block_len * baud));
  if (!(tb >= 2048.0) || !(tb <= 8192.0)) {
    kq_internal_set_error("%s: baud %g makes tb %.10g, a bit of %g frames of %u samples, outside 2048..8192 (8 to 32 frames)", fn,
                          baud, tb, tb / 256.0, b->cfg.block_len);
    return -1;
  }
  RttyPar np{};
  np.active = 1;
  np.source = p->source;
  np.inc_m = (unsigned)std::llrint(fm * 4294967296.0 / Fs);
  np.inc_s = (unsigned)std::llrint(fs * 4294967296.0 / Fs);
  np.tb = (int)tb;
  np.W = (np.tb + 128) >> 8;
  np.nbits = (int)p->nbits;
  b->nwant += !b->want[slot].active;
  b->want[slot] = np;
  b->touch(slot);
  return 0;
}

int kq_rtty_remove(kq_rtty_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_rtty_remove: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots || !b->want[slot].active) {
    kq_internal_set_error("kq_rtty_remove: slot %u holds no decoder", slot);
    return -1;
  }
  b->want[slot] = RttyPar{};
  b->nwant--;
  b->touch(slot);
  return 0;
}

int kq_rtty_process(kq_rtty_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_rtty_status *status, size_t status_stride) {
  if (!b) {
    kq_internal_set_error("kq_rtty_process: null bank");
    return -1;
  }
  if (format != KQ_PCM_F32 && format != KQ_PCM_S16BE) {
    kq_internal_set_error("kq_rtty_process: unknown sample format %d", format);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_rtty_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  if (status && status_stride < 1) {
    kq_internal_set_error("kq_rtty_process: status_stride %zu < 1", status_stride);
    return -1;
  }
  if (ncall == 0) return 0;
  if (!src) {
    kq_internal_set_error("kq_rtty_process: null src");
    return -1;
  }
  if (b->deviceless()) {
    (void)flush(b);
    b->n_cur += ncall;
    return 0;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (flush(b)) return -1;
  kq::CallWork const work = kq::call_work(b, "kq_rtty_process", ncall, src, "src");
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
  a.hist = d.hist;
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
  hipLaunchKernelGGL(k_rtty, dim3((unsigned)((nlist + kWaves - 1) / kWaves)), dim3(kThreads), 0, b->stream, a);
  KQ_TRY(hipGetLastError());
  b->n_cur += ncall;
  if (!on_device) {
    auto back = [&](size_t s0, size_t n) {  // the records of the active slots
      return kq::copy_rows_back(*b, status, status_stride, d.st, 1, 1, sizeof(kq_rtty_status), s0, n);
    };
    if (status && d.slots.for_runs(back)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  return 0;
}

int kq_rtty_pull_counts(kq_rtty_bank *b, uint32_t *counts) {
  if (!b) {
    kq_internal_set_error("kq_rtty_pull_counts: null bank");
    return -1;
  }
  if (!counts) {
    kq_internal_set_error("kq_rtty_pull_counts: null counts");
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

int kq_rtty_pull_event(kq_rtty_bank *b, unsigned slot, unsigned index, kq_rtty_event *event) {
  if (!b) {
    kq_internal_set_error("kq_rtty_pull_event: null bank");
    return -1;
  }
  if (!event) {
    kq_internal_set_error("kq_rtty_pull_event: null event");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots) {
    kq_internal_set_error("kq_rtty_pull_event: slot %u >= max_slots %u", slot, b->cfg.max_slots);
    return -1;
  }
  unsigned n = 0;
  if (b->deviceless()) {
    (void)flush(b);
    kq_internal_set_error("kq_rtty_pull_event: slot %u has %u events", slot, n);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (flush(b)) return -1;
  KQ_TRY(hipMemcpyAsync(&n, b->d.nev + slot, sizeof n, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  if (index >= n) {
    kq_internal_set_error("kq_rtty_pull_event: slot %u has %u events", slot, n);
    return -1;
  }
  size_t const at = (size_t)slot * b->cfg.max_events + index;
  KQ_TRY(hipMemcpyAsync(event, b->d.ev + at, sizeof *event, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_rtty_clear_events(kq_rtty_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_rtty_clear_events: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipMemsetAsync(b->d.nev, 0, b->cfg.max_slots * sizeof(unsigned), b->stream));
  return 0;
}

int kq_rtty_get_table(const kq_rtty_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_rtty_get_table: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_rtty_get_table: null dst");
    return -1;
  }
  size_t const n = std::min(cap, (size_t)kTable);
  if (n) std::memcpy(dst, cos_table().data(), n * sizeof(int16_t));
  return kTable;
}

int kq_rtty_get_slot(kq_rtty_bank *b, unsigned slot, kq_rtty_slot *out) {
  if (!b) {
    kq_internal_set_error("kq_rtty_get_slot: null bank");
    return -1;
  }
  if (!out) {
    kq_internal_set_error("kq_rtty_get_slot: null out");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_slots || !b->want[slot].active) {
    kq_internal_set_error("kq_rtty_get_slot: slot %u holds no decoder", slot);
    return -1;
  }
  RttyPar const &w = b->want[slot];
  out->inc_m = w.inc_m;
  out->inc_s = w.inc_s;
  out->tb = (uint32_t)w.tb;
  out->W = (uint32_t)w.W;
  return 0;
}

int kq_rtty_sync(kq_rtty_bank *b) { return kq::sync_bank(b, "kq_rtty_sync"); }

int kq_rtty_reset(kq_rtty_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_rtty_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  for (unsigned s = 0; s < b->cfg.max_slots; s++)  // every slot that is set starts cold at the next call
    if (b->want[s].active) b->touch(s);
  return 0;
}

}  // extern "C"
