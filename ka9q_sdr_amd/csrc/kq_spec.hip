// kq_spec.hip -- spectrum bank: averaged power spectra of the wideband I/Q stream on gfx950.
//
// Per analyzer (include/ka9q_hip.h, kq_spec_*): exact uint64 DDS mix, optional Kaiser-sinc decimation by Dz, Kaiser-windowed
// Nf-point frames every H decimated samples, |X|^2 of the B kept bins, K frames averaged into a row and corrected for the
// decimator's passband.  Every count of a call (decimated outputs, frames, rows) is a closed form of the stream index and
// the analyzer's start, so the host sizes the launches without reading anything back and the kernels find their work
// from the same formulas (spec_produced / spec_frames).
//
// k_spec_ingest   the call's samples converted (s16 / s8 / cf32, times gain_factor as k_ingest does) behind the last
//                 kHist samples of the previous call, into the other of two buffers (no overlap between source and target)
// k_spec_decim    one workgroup per (analyzer, tile of T decimated outputs): mixes the tile's input span into LDS in
//                 polyphase order (phase rho = i mod Dz in rows of Q, so the 64 lanes of a tap read 64 consecutive
//                 words), then one output per thread (two when the tile has <= 128 outputs: taps up to 12 Dz and the rest,
//                 added in that order), taps in ascending order; results into the analyzer's decimated ring
// k_spec_frames   one workgroup per (analyzer, frame completed in this call): window, kq::fft_any<-1> in LDS, |X|^2 of the
//                 kept bins into the analyzer's frame-power buffer
// k_spec_rows     one thread per (analyzer, kept bin): the call's frames added in frame order into the carried
//                 accumulator; a completed row is scaled by 1 / (K C[k] (sum w)^2) and written to the row ring (or dropped)
// A call whose frames exceed an analyzer's frame-power buffer runs frames + rows in rounds of `fcap` frames.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_ldsfft.hpp"

namespace {

using kq::FftDim;

constexpr unsigned kMaxSpecs = 4096;
constexpr int kMaxNf = 16384, kMinNf = 16, kMaxDz = 256;
constexpr int kGuard = 24;                        // Lh = kGuard Dz + 1 taps (Dz > 1)
constexpr int kHist = kGuard * kMaxDz;            // input samples kept from the previous call
constexpr size_t kFrameBudget = (size_t)1 << 21;  // frame-power floats per analyzer and round
constexpr int kTwLog2 = 14;                       // half-circle twiddles of period 16384 serve every power of two <= kMaxNf
constexpr double kTapBeta = 3.0;                  // the decimator's Kaiser window

struct SpecPar {  // per slot, written by the host at kq_spec_set / kq_spec_reset
  int active;
  int Dz, Nf, B, H, K;
  int G;          // kGuard when Dz > 1, else 0: Lh = G Dz + 1
  int T, Q;       // decimated outputs per k_spec_decim tile, LDS row length of one polyphase phase
  int R;          // decimated ring length
  int fcap;       // frames per round
  int max_rows;
  unsigned gen;
  int64_t s0;     // stream index where the analyzer started
  uint64_t inc, inc2;
  const float *taps;   // [Lh]
  const float *win;    // [Nf]
  const float *scale;  // [B] 1 / (K C[k] (sum w)^2)
  float2 *y;           // [R] decimated ring: y[j] at j mod R
  float *acc;          // [B] carried average
  float *fpow;         // [fcap][B]
  float *rows;         // [max_rows][B]
  kq_spec_row *meta;   // [max_rows]
  FftDim dN;
};
struct SpecCnt {  // rows put into the ring so far, rows pulled so far (the host writes `pulled` between calls)
  unsigned long long accepted, pulled;
};

// decimated outputs y[j] complete once the stream holds samples [0, n): y[j] needs x[s0 + j Dz]
__host__ __device__ inline uint64_t spec_produced(const SpecPar &p, uint64_t n) {
  int64_t const last = (int64_t)n - 1 - p.s0;
  return last < 0 ? 0 : (uint64_t)(last / p.Dz) + 1;
}
// frames complete once P decimated outputs are there
__host__ __device__ inline uint64_t spec_frames(const SpecPar &p, uint64_t P) {
  return P < (uint64_t)p.Nf ? 0 : (P - (uint64_t)p.Nf) / (uint64_t)p.H + 1;
}

struct CallArgs {
  const SpecPar *par;
  const SpecCnt *cnt_in;
  SpecCnt *cnt_out;
  const int *list;     // slots this launch serves
  const float2 *x;     // converted input: stream index n at x[n - (n0 - kHist)]
  uint64_t n0, n1;     // the call's samples [n0, n1)
  int round;
  const float2 *tw;
};

__global__ __launch_bounds__(256) void k_spec_ingest(const void *__restrict__ src, int format, float gain, size_t n,
                                                      const float2 *__restrict__ prev, size_t nprev, float2 *__restrict__ next) {
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < kHist + n; i += stride) {
    if (i < (size_t)kHist) {
      next[i] = prev[nprev + i];
      continue;
    }
    size_t const k = i - kHist;
    float2 v;
    if (format == KQ_IQ_S16) {
      short2 const q = reinterpret_cast<const short2 *>(src)[k];
      float const sc = 1.f / 32767.f;  // SCALE16, radio.c:38
      v = make_float2(q.x * sc, q.y * sc);
    } else if (format == KQ_IQ_S8) {
      char2 const q = reinterpret_cast<const char2 *>(src)[k];
      float const sc = 1.f / 127.f;  // SCALE8, radio.c:39
      v = make_float2(q.x * sc, q.y * sc);
    } else {
      v = reinterpret_cast<const float2 *>(src)[k];
    }
    next[i] = make_float2(v.x * gain, v.y * gain);  // radio.c:122
  }
}

// q = i / Dz, r = i mod Dz without an integer division (i < 2^24)
__device__ __forceinline__ void divmod_small(int i, int Dz, float inv, int &q, int &r) {
  q = (int)((float)i * inv);
  r = i - q * Dz;
  if (r < 0) {
    q--;
    r += Dz;
  } else if (r >= Dz) {
    q++;
    r -= Dz;
  }
}

// dynamic LDS: Dz rows of Q float2 (decim_lds_bytes)
__global__ __launch_bounds__(256) void k_spec_decim(CallArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 sm[];
  int const slot = a.list[blockIdx.y];
  SpecPar const &p = a.par[slot];
  uint64_t const J0 = spec_produced(p, a.n0), J1 = spec_produced(p, a.n1);
  uint64_t const jlo = J0 + (uint64_t)blockIdx.x * (uint64_t)p.T;
  if (jlo >= J1) return;
  int const nt = (int)min((uint64_t)p.T, J1 - jlo);
  int const Dz = p.Dz, G = p.G, Q = p.Q, tid = threadIdx.x, nthr = blockDim.x;
  // the tile's input span: stream samples nb .. nb + (nt - 1 + G) Dz
  int64_t const nb = p.s0 + (int64_t)jlo * Dz - (int64_t)G * Dz;
  int const span = (nt - 1 + G) * Dz + 1;
  const float2 *x = a.x + (nb - ((int64_t)a.n0 - kHist));
  float const inv = 1.f / (float)Dz;
  for (int i = tid; i < span; i += nthr) {
    int64_t const n = nb + i;
    int64_t const d = n - p.s0;
    // d (d - 1) / 2 exactly, then everything mod 2^64
    uint64_t const tri = (d & 1) ? (uint64_t)d * (uint64_t)((d - 1) / 2) : (uint64_t)(d / 2) * (uint64_t)(d - 1);
    uint64_t const ph = p.inc * (uint64_t)n + p.inc2 * tri;
    float const turns2 = (float)(int32_t)(uint32_t)(ph >> 32) * 0x1p-31f;  // 2 phi / 2^64 in [-1, 1)
    float s, c;
    sincospif(turns2, &s, &c);
    float2 const v = x[i];
    float2 const m = make_float2(v.x * c + v.y * s, v.y * c - v.x * s);  // x exp(-i 2 pi phi / 2^64)
    int q, r;
    divmod_small(i, Dz, inv, q, r);
    sm[r * Q + q] = m;
  }
  __syncthreads();
  // y[jlo + jj] = sum_t h[t] m[span index (jj + G) Dz - t]; tap t in ((c - 1) Dz, c Dz] lies in phase Dz - b (0 for b = Dz),
  // row position jj + G - c
  const float *h = p.taps;
  uint64_t const base = jlo % (uint64_t)p.R;
  // taps t = 0 (when with0) and rows c = c1 .. c2 of output jj
  auto fir = [&](int jj, bool with0, int c1, int c2, float &ax, float &ay) {
    if (with0) {
      float2 const v0 = sm[jj + G];
      ax = h[0] * v0.x;
      ay = h[0] * v0.y;
    }
    for (int c = c1; c <= c2; c++) {
      const float *hc = h + (c - 1) * Dz;
      const float2 *col = sm + (jj + G - c);
#pragma unroll 8
      for (int b = 1; b <= Dz; b++) {
        float2 const v = col[(Dz - b) * Q];
        float const hh = hc[b];
        ax = fmaf(hh, v.x, ax);
        ay = fmaf(hh, v.y, ay);
      }
    }
  };
  auto put = [&](int jj, float ax, float ay) {
    uint64_t pos = base + (uint64_t)jj;
    if (pos >= (uint64_t)p.R) pos -= p.R;
    p.y[pos] = make_float2(ax, ay);
  };
  if (G > 0 && 2 * p.T <= nthr) {
    // few outputs per tile (Dz >= 40): two threads per output, taps 0 .. G/2 Dz and the rest, added in that order
    __shared__ float2 red[128];
    int const half = nthr / 2, part = tid / half, jj = tid - part * half;
    float ax = 0.f, ay = 0.f;
    if (jj < nt) {
      if (part == 0)
        fir(jj, true, 1, G / 2, ax, ay);
      else
        fir(jj, false, G / 2 + 1, G, ax, ay);
    }
    if (part == 1 && jj < nt) red[jj] = make_float2(ax, ay);
    __syncthreads();
    if (part == 0 && jj < nt) put(jj, ax + red[jj].x, ay + red[jj].y);
  } else {
    for (int jj = tid; jj < nt; jj += nthr) {
      float ax = 0.f, ay = 0.f;
      fir(jj, true, 1, G, ax, ay);
      put(jj, ax, ay);
    }
  }
}

// dynamic LDS: Nf float2
__global__ __launch_bounds__(1024) void k_spec_frames(CallArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  int const slot = a.list[blockIdx.y];
  SpecPar const &p = a.par[slot];
  if ((int)blockIdx.x >= p.fcap) return;
  uint64_t const F0 = spec_frames(p, spec_produced(p, a.n0)), F1 = spec_frames(p, spec_produced(p, a.n1));
  uint64_t const f = F0 + (uint64_t)a.round * p.fcap + blockIdx.x;
  if (f >= F1) return;
  int const Nf = p.Nf, B = p.B, tid = threadIdx.x, nthr = blockDim.x;
  uint64_t const base = (f * (uint64_t)p.H) % (uint64_t)p.R;
  for (int i = tid; i < Nf; i += nthr) {
    uint64_t pos = base + (uint64_t)i;
    if (pos >= (uint64_t)p.R) pos -= p.R;
    float2 const v = p.y[pos];
    float const w = p.win[i];
    buf[kq::fft_pos((unsigned)i, p.dN)] = make_float2(v.x * w, v.y * w);
  }
  kq::fft_any<-1>(buf, p.dN, a.tw, kTwLog2);
  float *dst = p.fpow + (size_t)blockIdx.x * B;
  for (int j = tid; j < B; j += nthr) {
    int const k = j - B / 2;
    dst[j] = kq::cnrm(buf[k < 0 ? k + Nf : k]);
  }
}

// grid (bin tiles of 256, analyzers).  The row counter is read from cnt_in and written to cnt_out (the host swaps the two
// halves every launch), so no workgroup reads what another one of the same launch writes
__global__ __launch_bounds__(256) void k_spec_rows(CallArgs a) {
  int const slot = a.list[blockIdx.y];
  SpecPar const &p = a.par[slot];
  SpecCnt const c0 = a.cnt_in[slot];
  uint64_t const F0 = spec_frames(p, spec_produced(p, a.n0)), F1 = spec_frames(p, spec_produced(p, a.n1));
  uint64_t const flo = F0 + (uint64_t)a.round * p.fcap;
  bool const writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (flo >= F1) {
    if (writer) a.cnt_out[slot] = c0;
    return;
  }
  uint64_t const fhi = min(F1, flo + (uint64_t)p.fcap);
  int const B = p.B, K = p.K, j = blockIdx.x * blockDim.x + threadIdx.x;
  bool const mine = j < B;
  float acc = mine ? p.acc[j] : 0.f;
  float const sc = mine ? p.scale[j] : 0.f;
  unsigned long long accepted = c0.accepted;
  int fk = (int)(flo % (uint64_t)K);
  for (uint64_t f = flo; f < fhi; f++) {
    float const v = mine ? p.fpow[(size_t)(f - flo) * B + j] : 0.f;
    acc = fk == 0 ? v : acc + v;
    if (++fk == K) {
      fk = 0;
      if (accepted - c0.pulled < (unsigned long long)p.max_rows) {
        unsigned long long const r = accepted % (unsigned long long)p.max_rows;
        if (mine) p.rows[r * B + j] = acc * sc;
        if (writer) {
          uint64_t const row = f / (uint64_t)K;
          kq_spec_row m;
          m.start_sample = (uint64_t)p.s0 + row * (uint64_t)K * (uint64_t)p.H * (uint64_t)p.Dz;
          m.frames = (uint32_t)K;
          m.generation = p.gen;
          p.meta[r] = m;
        }
        accepted++;
      }
    }
  }
  if (mine) p.acc[j] = acc;
  if (writer) a.cnt_out[slot] = SpecCnt{accepted, c0.pulled};
}

size_t decim_lds_bytes(int Dz, int Q) { return (size_t)Dz * Q * sizeof(float2); }

// filter.c:282-293 and 337-357 in the reference's own float arithmetic (the window of every frame)
float i0f_ref(float const x) {
#pragma clang fp contract(off)
  const float t = 0.25 * x * x;
  float sum = 1 + t;
  float term = t;
  for (int k = 2; k < 40; k++) {
    term *= t / (k * k);
    sum += term;
    if (term < 1e-12 * sum) break;
  }
  return sum;
}
void make_kaiser_ref(float *window, unsigned M, float beta) {
#pragma clang fp contract(off)
  float const numc = M_PI * beta;
  float const inv_denom = 1. / i0f_ref(numc);
  float const pc = 2.0 / (M - 1);
  for (int n = 0; n < (int)(M / 2); n++) {
    float const p = pc * n - 1;
    window[M - 1 - n] = window[n] = i0f_ref(numc * sqrtf(1 - p * p)) * inv_denom;
  }
  if (M & 1) window[(M - 1) / 2] = 1;
}

// h[t] = g kaiser(Lh, 3.0)[t] sinc((t - G Dz / 2) / Dz), sum h = 1, designed in double (symmetric by construction), float
std::vector<float> design_taps(int Dz) {
  if (Dz == 1) return {1.f};
  int const Lh = kGuard * Dz + 1, c = kGuard * Dz / 2;
  std::vector<double> h(Lh);
  double const a = M_PI * kTapBeta, den = kq::i0_double(a);
  double sum = 0;
  for (int t = 0; t < Lh; t++) {
    int const u = std::abs(t - c);
    double const pp = (double)u / c;  // |2 t / (Lh - 1) - 1|
    double const w = kq::i0_double(a * std::sqrt(std::max(0.0, 1.0 - pp * pp))) / den;
    double const xx = (double)u / Dz;
    double const sinc = u == 0 ? 1.0 : std::sin(M_PI * xx) / (M_PI * xx);
    h[t] = w * sinc;
    sum += h[t];
  }
  std::vector<float> out(Lh);
  for (int t = 0; t < Lh; t++) out[t] = (float)(h[t] / sum);
  return out;
}

// C[k] = |H(k / (Dz Nf))|^2 of the float taps, k = -B/2 .. B/2 - 1 (symmetric taps: H = e^{-i..} (h_c + 2 sum h_{c+u} cos))
std::vector<double> taps_power(const std::vector<float> &h, int Dz, int Nf, int B) {
  std::vector<double> C(B, 1.0);
  if (Dz == 1) return C;
  int const c = (int)h.size() / 2;
  for (int j = 0; j < B; j++) {
    double const th = 2 * M_PI * (double)(j - B / 2) / ((double)Dz * Nf);
    double const c1 = std::cos(th);
    double cm2 = 1.0, cm1 = c1, A = h[c] + 2.0 * h[c + 1] * c1;  // cos(0 th), cos(1 th)
    for (int u = 2; u <= c; u++) {
      double const cu = 2 * c1 * cm1 - cm2;
      A += 2.0 * h[c + u] * cu;
      cm2 = cm1;
      cm1 = cu;
    }
    C[j] = A * A;
  }
  return C;
}

uint64_t dds_word(double cycles_per_sample) {  // round(v 2^64) mod 2^64, |v| <= 1/2
  double v = std::rint(std::ldexp(cycles_per_sample, 64));
  if (v >= 0x1p63) v -= 0x1p64;
  return (uint64_t)(int64_t)v;
}

struct SlotMem {
  float *taps = nullptr, *win = nullptr, *scale = nullptr, *acc = nullptr, *fpow = nullptr, *rows = nullptr;
  float2 *y = nullptr;
  kq_spec_row *meta = nullptr;
  int rowsB = 0;  // row width the row ring holds
};

struct Group {  // analyzers of one (Dz, Nf): one k_spec_decim and one k_spec_frames launch per call
  int Dz, Nf, T, Q, dthreads, fthreads;
  int off, n;   // in the device list
  std::vector<int> slots;
};

}  // namespace

struct kq_spec_bank : kq::HostSide {
  kq_spec_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  // stream state
  uint64_t n_cur = 0;  // samples taken since create / reset
  size_t nprev = 0;    // samples of the last call (the history is the last kHist of xbuf[cur])
  int cur = 0;
  // host mirror
  std::vector<SpecPar> par;
  std::vector<kq_spec_params> prm;
  std::vector<SpecCnt> cnt;
  std::vector<unsigned long long> dropped;
  std::vector<unsigned> gen;
  std::vector<double> enbw;
  std::vector<SlotMem> mem;
  std::vector<Group> groups;
  std::vector<int> all;  // active slots, ascending
  int maxB = 0;          // widest row among them
  int cnt_half = 0;      // the half of d.cnt the next k_spec_rows reads
  const float2 *tw = nullptr;  // kq::half_twiddles(kTwLog2): shared, not the bank's to free
  struct Dev {  // kq::lazy_device (the slots' own memory, `mem`, comes and goes with each slot)
    SpecPar *par = nullptr;
    SpecCnt *cnt = nullptr;  // [2][S]: k_spec_rows reads one half and writes the other
    int *list = nullptr;     // [all | group lists]
    float2 *xbuf[2] = {nullptr, nullptr};
    float2 *raw = nullptr;   // [max_samples] a host-memory call's samples as they came, whatever their format
  } d;
};

namespace {

int make_device(kq_spec_bank *b) {
  kq_spec_config const &c = b->cfg;
  if (b->open_stream(c.stream)) return -1;
  size_t const S = c.max_specs, X = kHist + c.max_samples;
  if (!(b->tw = kq::half_twiddles(kTwLog2))) {
    kq_internal_set_error("kq_spec: no twiddle table of period 2^%d", kTwLog2);
    return -1;
  }
  if (b->alloc(&b->d.par, S, true) || b->alloc(&b->d.cnt, 2 * S, true) || b->alloc(&b->d.list, 2 * S) ||
      b->alloc(&b->d.xbuf[0], X, true) || b->alloc(&b->d.xbuf[1], X, true) || b->alloc(&b->d.raw, c.max_samples))
    return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

void free_slot_mem(kq_spec_bank *b, SlotMem &m, bool rows_too) {
  b->release(&m.taps, &m.win, &m.scale, &m.acc, &m.fpow, &m.y);
  if (rows_too) {
    b->release(&m.rows, &m.meta);
    m.rowsB = 0;
  }
}

// the active-slot list and the (Dz, Nf) groups, uploaded (the stream is idle: callers synchronised it)
int rebuild_lists(kq_spec_bank *b) {
  b->all.clear();
  b->maxB = 0;
  std::map<std::pair<int, int>, int> gi;
  b->groups.clear();
  for (unsigned s = 0; s < b->cfg.max_specs; s++) {
    SpecPar const &p = b->par[s];
    if (!p.active) continue;
    b->all.push_back((int)s);
    b->maxB = std::max(b->maxB, p.B);
    auto key = std::make_pair(p.Dz, p.Nf);
    auto it = gi.find(key);
    if (it == gi.end()) {
      Group g{};
      g.Dz = p.Dz;
      g.Nf = p.Nf;
      g.T = p.T;
      g.Q = p.Q;
      g.dthreads = 256;
      g.fthreads = kq::fft_threads(p.Nf);
      it = gi.emplace(key, (int)b->groups.size()).first;
      b->groups.push_back(g);
    }
    b->groups[it->second].slots.push_back((int)s);
  }
  std::vector<int> list(b->all);
  for (Group &g : b->groups) {
    g.off = (int)list.size();
    g.n = (int)g.slots.size();
    list.insert(list.end(), g.slots.begin(), g.slots.end());
  }
  if (!list.empty()) KQ_TRY(hipMemcpy(b->d.list, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

int upload_slot(kq_spec_bank *b, unsigned s) {
  KQ_TRY(hipMemcpyAsync(b->d.par + s, &b->par[s], sizeof(SpecPar), hipMemcpyHostToDevice, b->stream));
  for (int h = 0; h < 2; h++)
    KQ_TRY(hipMemcpyAsync(b->d.cnt + h * b->cfg.max_specs + s, &b->cnt[s], sizeof(SpecCnt), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

const char *check_params(const kq_spec_params *p) {
  static thread_local char why[160];
  unsigned const Dz = p->decimate, Nf = p->fft_size, B = p->bins;
  if (!std::isfinite(p->center)) return "center is not finite";
  if (!std::isfinite(p->sweep)) return "sweep is not finite";
  if (Dz < 1 || Dz > (unsigned)kMaxDz) {
    snprintf(why, sizeof why, "decimate %u must be 1..%d", Dz, kMaxDz);
    return why;
  }
  if (Nf < (unsigned)kMinNf || Nf > (unsigned)kMaxNf || (Nf & 1) || !kq::fft_size_ok((int)Nf)) {
    snprintf(why, sizeof why, "fft_size %u must be even, 2^a 3^b 5^c 7^d and %d..%d", Nf, kMinNf, kMaxNf);
    return why;
  }
  if (B == 0 || (B & 1)) {
    snprintf(why, sizeof why, "bins %u must be even and positive", B);
    return why;
  }
  if (Dz == 1 && B > Nf) {
    snprintf(why, sizeof why, "bins %u > fft_size %u", B, Nf);
    return why;
  }
  if (Dz > 1 && 4 * (unsigned long)B > 3 * (unsigned long)Nf) {
    snprintf(why, sizeof why, "bins %u > 3 fft_size / 4 = %u at decimate %u (the rest is the decimator's transition band)", B,
             3 * Nf / 4, Dz);
    return why;
  }
  if (p->hop < 1 || p->hop > Nf) {
    snprintf(why, sizeof why, "hop %u must be 1..fft_size %u", p->hop, Nf);
    return why;
  }
  if (p->average < 1) return "average must be >= 1";
  if (!std::isfinite(p->kaiser_beta) || p->kaiser_beta < 0) return "kaiser_beta must be finite and >= 0";
  return nullptr;
}

}  // namespace

extern "C" {

kq_spec_bank *kq_spec_create(const kq_spec_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_spec_create: null config");
    return nullptr;
  }
  if (cfg->samprate <= 0) {
    kq_internal_set_error("kq_spec_create: samprate %d must be positive", cfg->samprate);
    return nullptr;
  }
  if (!std::isfinite(cfg->gain_factor)) {
    kq_internal_set_error("kq_spec_create: gain_factor is not finite");
    return nullptr;
  }
  if (cfg->max_specs == 0 || cfg->max_specs > kMaxSpecs) {
    kq_internal_set_error("kq_spec_create: max_specs %u must be 1..%u", cfg->max_specs, kMaxSpecs);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_spec_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  if (cfg->max_rows == 0) {
    kq_internal_set_error("kq_spec_create: max_rows must be positive");
    return nullptr;
  }
  kq_spec_bank *b = new kq_spec_bank;
  b->cfg = *cfg;
  size_t const S = cfg->max_specs;
  b->par.assign(S, SpecPar{});
  b->prm.assign(S, kq_spec_params{});
  b->cnt.assign(S, SpecCnt{});
  b->dropped.assign(S, 0);
  b->gen.assign(S, 0);
  b->enbw.assign(S, 0.0);
  b->mem.assign(S, SlotMem{});
  return b;
}

int kq_spec_destroy(kq_spec_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_spec_destroy: null bank");
    return -1;
  }
  if (b->dev_ready) {
    kq::DeviceScope dev_scope_(b->cfg.device);
    b->close();
  }
  delete b;
  return 0;
}

int kq_spec_set(kq_spec_bank *b, unsigned slot, const kq_spec_params *p) {
  if (slot >= kMaxSpecs) {
    kq_internal_set_error("kq_spec_set: slot %u is beyond any bank (%u analyzers at most)", slot, kMaxSpecs);
    return -1;
  }
  if (!p) {
    kq_internal_set_error("kq_spec_set: null params");
    return -1;
  }
  if (const char *why = check_params(p)) {
    kq_internal_set_error("kq_spec_set: %s", why);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_spec_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_specs) {
    kq_internal_set_error("kq_spec_set: slot %u >= max_specs %u", slot, b->cfg.max_specs);
    return -1;
  }
  double const Fs = (double)b->cfg.samprate;
  if (std::fabs(p->center) > Fs / 2) {
    kq_internal_set_error("kq_spec_set: center %g Hz is out of band (|center| <= samprate / 2 = %g)", p->center, Fs / 2);
    return -1;
  }
  if (std::fabs(p->sweep) >= Fs * Fs / 2) {
    kq_internal_set_error("kq_spec_set: sweep %g Hz/s must be below samprate^2 / 2", p->sweep);
    return -1;
  }
  bool okN = false;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  FftDim const dN = kq::fft_dim((int)p->fft_size, &okN);
  if (!okN) {
    kq_internal_set_error("kq_spec_set: no transform plan for fft_size %u", p->fft_size);
    return -1;
  }
  KQ_TRY(hipStreamSynchronize(b->stream));
  int const Dz = (int)p->decimate, Nf = (int)p->fft_size, B = (int)p->bins, H = (int)p->hop, K = (int)p->average;
  int const G = Dz > 1 ? kGuard : 0;
  size_t const max_new = (b->cfg.max_samples + Dz - 1) / Dz;
  SpecPar np{};
  np.active = 1;
  np.Dz = Dz;
  np.Nf = Nf;
  np.B = B;
  np.H = H;
  np.K = K;
  np.G = G;
  np.T = std::min(1024, std::max(32, 8191 / Dz - G));
  np.Q = (np.T + G) | 1;  // odd: the staging writes of consecutive samples spread over the banks
  np.R = (int)(Nf + max_new + 1);
  np.fcap = (int)std::min<size_t>(max_new / H + 1, std::max<size_t>(1, kFrameBudget / B));
  np.max_rows = (int)b->cfg.max_rows;
  np.gen = ++b->gen[slot];
  np.s0 = (int64_t)b->n_cur;
  np.inc = dds_word(p->center / Fs);
  np.inc2 = dds_word(p->sweep / (Fs * Fs));
  np.dN = dN;
  // host tables
  std::vector<float> taps = design_taps(Dz), win(Nf);
  make_kaiser_ref(win.data(), (unsigned)Nf, p->kaiser_beta);
  double sw = 0, sw2 = 0;
  for (float w : win) {
    sw += w;
    sw2 += (double)w * w;
  }
  std::vector<double> C = taps_power(taps, Dz, Nf, B);
  std::vector<float> scale(B);
  for (int j = 0; j < B; j++) scale[j] = (float)(1.0 / ((double)K * C[j] * sw * sw));
  // device memory of the slot; the row ring stays when B does
  SlotMem &m = b->mem[slot];
  bool const was = b->par[slot].active != 0;
  unsigned long long const unpulled = b->cnt[slot].accepted - b->cnt[slot].pulled;
  bool const keep_rows = was && m.rowsB == B;
  if (!was) b->dropped[slot] = 0;
  free_slot_mem(b, m, !keep_rows);
  if (!keep_rows) {
    if (was) b->dropped[slot] += unpulled;
    b->cnt[slot] = SpecCnt{};
    if (b->alloc(&m.rows, (size_t)b->cfg.max_rows * B) || b->alloc(&m.meta, (size_t)b->cfg.max_rows)) return -1;
    m.rowsB = B;
  }
  if (b->alloc(&m.taps, taps.size()) || b->alloc(&m.win, (size_t)Nf) || b->alloc(&m.scale, (size_t)B) ||
      b->alloc(&m.acc, (size_t)B, true) || b->alloc(&m.fpow, (size_t)np.fcap * B) || b->alloc(&m.y, (size_t)np.R))
    return -1;
  KQ_TRY(hipMemcpyAsync(m.taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipMemcpyAsync(m.win, win.data(), (size_t)Nf * sizeof(float), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipMemcpyAsync(m.scale, scale.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, b->stream));
  np.taps = m.taps;
  np.win = m.win;
  np.scale = m.scale;
  np.acc = m.acc;
  np.fpow = m.fpow;
  np.y = m.y;
  np.rows = m.rows;
  np.meta = m.meta;
  b->par[slot] = np;
  b->prm[slot] = *p;
  b->enbw[slot] = (double)Nf * sw2 / (sw * sw);
  if (upload_slot(b, slot)) return -1;
  return rebuild_lists(b);
}

int kq_spec_remove(kq_spec_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_spec_remove: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_specs || !b->par[slot].active) {
    kq_internal_set_error("kq_spec_remove: slot %u holds no analyzer", slot);
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  free_slot_mem(b, b->mem[slot], true);
  b->par[slot] = SpecPar{};
  b->cnt[slot] = SpecCnt{};
  if (upload_slot(b, slot)) return -1;
  return rebuild_lists(b);
}

int kq_spec_process(kq_spec_bank *b, const void *iq, int format, size_t nsamples, int on_device) {
  if (format != KQ_IQ_CF32 && format != KQ_IQ_S16 && format != KQ_IQ_S8) {
    kq_internal_set_error("kq_spec_process: unknown format %d (KQ_IQ_CF32, KQ_IQ_S16 or KQ_IQ_S8)", format);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_spec_process: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (nsamples > b->cfg.max_samples) {
    kq_internal_set_error("kq_spec_process: nsamples %zu > max_samples %zu", nsamples, b->cfg.max_samples);
    return -1;
  }
  if (nsamples == 0) return 0;
  if (!iq) {
    kq_internal_set_error("kq_spec_process: null iq");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  size_t const esize = format == KQ_IQ_CF32 ? 8 : format == KQ_IQ_S16 ? 4 : 2;
  const void *src = iq;
  if (!on_device) {
    KQ_TRY(hipMemcpyAsync(b->d.raw, iq, nsamples * esize, hipMemcpyHostToDevice, b->stream));
    src = b->d.raw;
  }
  int const nxt = b->cur ^ 1;
  {
    size_t const total = kHist + nsamples;
    unsigned const blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_spec_ingest, dim3(blocks), dim3(256), 0, b->stream, src, format, b->cfg.gain_factor, nsamples,
                       (const float2 *)b->d.xbuf[b->cur], b->nprev, b->d.xbuf[nxt]);
    KQ_TRY(hipGetLastError());
  }
  uint64_t const n0 = b->n_cur, n1 = n0 + nsamples;
  CallArgs a{};
  a.par = b->d.par;
  a.x = b->d.xbuf[nxt];
  a.n0 = n0;
  a.n1 = n1;
  a.tw = b->tw;
  int rounds = 0;
  for (Group const &g : b->groups) {
    uint64_t tiles = 0;
    for (int s : g.slots) {
      SpecPar const &p = b->par[s];
      uint64_t const nj = spec_produced(p, n1) - spec_produced(p, n0);
      tiles = std::max<uint64_t>(tiles, (nj + p.T - 1) / p.T);
      uint64_t const nf = spec_frames(p, spec_produced(p, n1)) - spec_frames(p, spec_produced(p, n0));
      rounds = std::max<int>(rounds, (int)((nf + p.fcap - 1) / p.fcap));
    }
    if (!tiles) continue;
    a.list = b->d.list + g.off;
    size_t const lds = decim_lds_bytes(g.Dz, g.Q);
    kq::ensure_dynamic_lds((const void *)k_spec_decim, lds);
    hipLaunchKernelGGL(k_spec_decim, dim3((unsigned)tiles, (unsigned)g.n), dim3(g.dthreads), lds, b->stream, a);
    KQ_TRY(hipGetLastError());
  }
  for (int r = 0; r < rounds; r++) {
    a.round = r;
    for (Group const &g : b->groups) {
      uint64_t fr = 0;
      for (int s : g.slots) {
        SpecPar const &p = b->par[s];
        uint64_t const nf = spec_frames(p, spec_produced(p, n1)) - spec_frames(p, spec_produced(p, n0));
        uint64_t const done = (uint64_t)r * p.fcap;
        if (nf > done) fr = std::max<uint64_t>(fr, std::min<uint64_t>(nf - done, p.fcap));
      }
      if (!fr) continue;
      a.list = b->d.list + g.off;
      size_t const lds = (size_t)g.Nf * sizeof(float2);
      kq::ensure_dynamic_lds((const void *)k_spec_frames, lds);
      hipLaunchKernelGGL(k_spec_frames, dim3((unsigned)fr, (unsigned)g.n), dim3(g.fthreads), lds, b->stream, a);
      KQ_TRY(hipGetLastError());
    }
    a.list = b->d.list;
    a.cnt_in = b->d.cnt + (size_t)b->cnt_half * b->cfg.max_specs;
    a.cnt_out = b->d.cnt + (size_t)(b->cnt_half ^ 1) * b->cfg.max_specs;
    hipLaunchKernelGGL(k_spec_rows, dim3((unsigned)((b->maxB + 255) / 256), (unsigned)b->all.size()), dim3(256), 0, b->stream, a);
    KQ_TRY(hipGetLastError());
    b->cnt_half ^= 1;
  }
  // the host's account of the rows, by the rule k_spec_rows applies
  for (int s : b->all) {
    SpecPar const &p = b->par[s];
    uint64_t const r0 = spec_frames(p, spec_produced(p, n0)) / p.K, r1 = spec_frames(p, spec_produced(p, n1)) / p.K;
    unsigned long long const fresh = r1 - r0, room = (unsigned long long)p.max_rows - (b->cnt[s].accepted - b->cnt[s].pulled);
    unsigned long long const take = std::min(fresh, room);
    b->cnt[s].accepted += take;
    b->dropped[s] += fresh - take;
  }
  b->n_cur = n1;
  b->nprev = nsamples;
  b->cur = nxt;
  if (!on_device) KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_spec_pull(kq_spec_bank *b, unsigned slot, float *rows, unsigned max_rows, kq_spec_row *meta) {
  if (!b) {
    kq_internal_set_error("kq_spec_pull: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_specs || !b->par[slot].active) {
    kq_internal_set_error("kq_spec_pull: slot %u holds no analyzer", slot);
    return -1;
  }
  if (!rows && max_rows) {
    kq_internal_set_error("kq_spec_pull: null rows");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  SpecCnt &c = b->cnt[slot];
  SlotMem const &m = b->mem[slot];
  unsigned long long const ready = c.accepted - c.pulled;
  unsigned const n = (unsigned)std::min<unsigned long long>(ready, max_rows);
  size_t const B = (size_t)m.rowsB, cap = b->cfg.max_rows;
  for (unsigned i = 0; i < n;) {  // at most two runs: up to the end of the ring, then from its start
    size_t const r = (size_t)((c.pulled + i) % cap);
    unsigned const run = (unsigned)std::min<size_t>(n - i, cap - r);
    KQ_TRY(hipMemcpyAsync(rows + (size_t)i * B, m.rows + r * B, (size_t)run * B * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (meta) KQ_TRY(hipMemcpyAsync(meta + i, m.meta + r, run * sizeof(kq_spec_row), hipMemcpyDeviceToHost, b->stream));
    i += run;
  }
  c.pulled += n;
  for (int h = 0; h < 2; h++)
    KQ_TRY(hipMemcpyAsync(b->d.cnt + h * b->cfg.max_specs + slot, &c, sizeof c, hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return (int)n;
}

int kq_spec_get_info(kq_spec_bank *b, unsigned slot, kq_spec_info *out) {
  if (!b || !out) {
    kq_internal_set_error("kq_spec_get_info: null %s", b ? "out" : "bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_specs || !b->par[slot].active) {
    kq_internal_set_error("kq_spec_get_info: slot %u holds no analyzer", slot);
    return -1;
  }
  SpecPar const &p = b->par[slot];
  double const Fs = (double)b->cfg.samprate;
  kq_spec_info i{};
  i.bin_bw = Fs / ((double)p.Dz * p.Nf);
  i.first_bin_hz = b->prm[slot].center - (double)(p.B / 2) * i.bin_bw;
  i.enbw_bins = b->enbw[slot];
  i.delay_samples = p.Dz > 1 ? 0.5 * kGuard * p.Dz : 0.0;
  i.rows_ready = b->cnt[slot].accepted - b->cnt[slot].pulled;
  i.rows_dropped = b->dropped[slot];
  i.frames_pending = (uint32_t)(spec_frames(p, spec_produced(p, b->n_cur)) % (uint64_t)p.K);
  i.generation = p.gen;
  *out = i;
  return 0;
}

int kq_spec_sync(kq_spec_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_spec_sync: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_spec_reset(kq_spec_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_spec_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  b->nprev = 0;
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  size_t const X = kHist + b->cfg.max_samples;
  for (auto &p : b->d.xbuf) KQ_TRY(hipMemsetAsync(p, 0, X * sizeof(float2), b->stream));
  for (int s : b->all) {
    b->par[s].s0 = 0;
    b->cnt[s] = SpecCnt{};
    KQ_TRY(hipMemsetAsync(b->mem[s].acc, 0, (size_t)b->par[s].B * sizeof(float), b->stream));
  }
  KQ_TRY(hipMemcpyAsync(b->d.par, b->par.data(), b->par.size() * sizeof(SpecPar), hipMemcpyHostToDevice, b->stream));
  for (int h = 0; h < 2; h++)
    KQ_TRY(hipMemcpyAsync(b->d.cnt + h * b->cfg.max_specs, b->cnt.data(), b->cnt.size() * sizeof(SpecCnt), hipMemcpyHostToDevice,
                            b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // extern "C"
