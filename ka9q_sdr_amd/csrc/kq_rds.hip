// kq_rds.hip -- RDS / RBDS decoder bank: broadcast FM composite -> the 57 kHz data subcarrier's groups on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_rds_*): z[k] = (h_r * x)[k Dr] exp(-j 2 pi 57000 k Dr / Fc), the matched-filtered
// subcarrier at Fr = Fc / Dr; per frame the sums S = sum z^2, E = sum |z|^2 exp(-j 2 pi 1187.5 k / Fr), P = sum |z|^2;
// a first-order tracker of the carrier phase (arg S / 2) and the bit clock (-arg E / 2 pi); bits by linear interpolation
// of z at the tracked instants, differential decoding, and the 26-bit block / group machine.  Frames are L samples on a
// grid shared by every slot, as in kq_wfm.hip, so the host sizes the launches without reading anything back.  State on the
// device, per slot: a ring of the composite (x[n] at n mod Rx), a ring of z (z[k] at k mod Rz, the call's samples and the
// ceil(spb) + 2 before them that the interpolator may reach back to), the frame sums of the call, the carried RdsState.
//
// k_rds_ingest  the call's composite samples of each slot's source row into the slot's ring
// k_rds_front   one workgroup per (slot, frame): x's N-window, kq::fft_any<-1> in LDS, times H_r folded to Nr = N / Dr bins
//               that start at the subcarrier's bin (exact decimation: the aliases are added; the shift is the mix to
//               baseband), Nr-point inverse transform, the frame's phase, Lr samples into the z ring, the three sums
// k_rds_track   one lane per slot: the call's frames in order through tracker, bit sampler, differential decoder and
//               block / group machine; status and groups out.  Serial by nature (each bit's instant and each block's
//               place depend on everything before), as k_afsk's deframer is
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <complex>
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
#include "kq_slots.hpp"
#include "kq_window.hpp"

namespace {

using kq::FftDim;

constexpr unsigned kMaxSlots = 4096;
constexpr int kMaxN = 16384;
constexpr int kTwLog2 = 14;      // half-circle twiddles of period 16384 serve every power of two <= kMaxN
constexpr int kPer = 16;         // transform points per thread at most (kq::fft_threads)
constexpr int kSubHz = 57000;
constexpr double kBitHz = 1187.5;
constexpr int kSums = 5;         // Re S, Im S, Re E, Im E, P

struct RdsPar {  // per slot, written by the host at kq_rds_set
  int active;
  unsigned source;
  int lose_after;
  int pad;
  double alpha;                  // 1 - exp(-L / (Fc track_ms 1e-3))
};

struct RdsState {  // per slot, carried from call to call; all zero when a slot is set
  double ar, ai, br, bi;         // A, B
  double phi, tau;
  long long next_i;              // the next unsampled bit
  int started;
  int cprev;
  unsigned reg, nbits;
  int synced, expect;
  unsigned next_at;
  int bad;
  int rem_valid, rem_pos, rem_cp;
  unsigned rem_nbits, rem_info;
  unsigned blocks_ok, blocks_bad;
  unsigned ok, vb;
  unsigned long long blk;        // the open record's four words, position p at bits 16 p
};

struct RdsGeom {
  int N, L, M, Dr, Nr, Lr, skip;  // Lr = L / Dr samples of z per frame, skip = (M - 1) / Dr
  int nthr;
  int Fmax;
  int Fc, Fr, k0;                 // k0 = 57000 N / Fc: the subcarrier's bin
  size_t Rx, Rz;
  double spb;                     // Fr / 1187.5
  FftDim dN, dNr;
  const float2 *tw;
  const float2 *hr;               // [N] H_r / N
};

struct CallArgs {
  RdsGeom g;
  const RdsPar *par;
  const int *list;                // active slots, ascending
  float *x;                       // [S][Rx]
  float2 *z;                      // [S][Rz]
  double *sums;                   // [S][Fmax][kSums]
  RdsState *state;                // [S]
  uint64_t n0, F0;                // the call's first sample, first frame
  int F;
  // input
  const float *comp;
  size_t src_stride, row_stride;
  unsigned block_len;
  const int *rowmap;              // per list entry: the row of `comp` (host input, staged) or null (par.source)
  size_t xbase;                   // n0 mod Rx
  // output
  kq_rds_group *groups;
  size_t gstride;
  unsigned gcap;                  // groups per slot this call may write
  uint32_t *counts;
  kq_rds_status *st;
  size_t sstride;
};

__device__ __forceinline__ size_t ring_pos(int64_t n, size_t R) {
  int64_t const r = n % (int64_t)R;
  return (size_t)(r < 0 ? r + (int64_t)R : r);
}

__global__ __launch_bounds__(256) void k_rds_ingest(CallArgs a, size_t ncall) {
  int const li = blockIdx.y, slot = a.list[li];
  size_t const row = a.rowmap ? (size_t)a.rowmap[li] : (size_t)a.par[slot].source;
  const float *src = a.comp + row * a.src_stride;
  float *x = a.x + (size_t)slot * a.g.Rx;
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncall; i += stride) {
    size_t const k = i / a.block_len, j = i - k * a.block_len;
    size_t pos = a.xbase + i;
    if (pos >= a.g.Rx) pos -= a.g.Rx;
    x[pos] = src[k * a.row_stride + j];
  }
}

// sums of kSums doubles over the workgroup, in a fixed order (every thread gets them)
__device__ void block_sums(double (&v)[kSums], double *red) {
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int c = 0; c < kSums; c++) v[c] += __shfl_xor(v[c], m);
  }
  int const wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < kSums; c++) red[kSums * wv + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kSums; c++) v[c] = 0.0;
  for (int k = 0; k < nw; k++) {
#pragma unroll
    for (int c = 0; c < kSums; c++) v[c] += red[kSums * k + c];
  }
}

// dynamic LDS: N float2
__global__ __launch_bounds__(1024) void k_rds_front(CallArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  __shared__ double red[kSums * 16];
  RdsGeom const &g = a.g;
  int const slot = a.list[blockIdx.y], fi = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  int64_t const f = (int64_t)(a.F0 + (uint64_t)fi);
  const float *x = a.x + (size_t)slot * g.Rx;
  float2 *zr = a.z + (size_t)slot * g.Rz;
  // window: x[f L - (M - 1) + i], i < N
  int64_t const w0 = f * g.L - (g.M - 1);
  size_t const px = ring_pos(w0, g.Rx);
  for (int i = tid; i < g.N; i += nthr) {
    size_t pos = px + i;
    if (pos >= g.Rx) pos -= g.Rx;
    buf[kq::fft_pos((unsigned)i, g.dN)] = make_float2(x[pos], 0.f);
  }
  kq::fft_any<-1>(buf, g.dN, g.tw, kTwLog2);
  // Y[q] = sum_r X[b + r Nr] H_r[b + r Nr], b = (q + k0) mod Nr, q < Nr: the N-point output at every Dr-th sample, times
  // exp(-j 2 pi k0 i / N) at window index i
  {
    float2 v[kPer];
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const q = tid + t * nthr;
      if (q < g.Nr) {
        int const b = (q + g.k0) % g.Nr;
        float2 acc = make_float2(0.f, 0.f);
        for (int r = 0; r < g.Dr; r++) {
          int const kk = b + r * g.Nr;
          acc = kq::cadd(acc, kq::cmul(buf[kk], g.hr[kk]));
        }
        v[t] = acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPer; t++) {
      int const q = tid + t * nthr;
      if (q < g.Nr) buf[kq::fft_pos((unsigned)q, g.dNr)] = v[t];
    }
  }
  kq::fft_any<+1>(buf, g.dNr, g.tw, kTwLog2);
  // the window's first sample carries the phase -2 pi k0 w0 / N, kept exact by integer arithmetic
  float2 rot;
  {
    int64_t m = w0 % g.N;
    if (m < 0) m += g.N;
    int const e = (int)(((int64_t)g.k0 * m) % g.N);
    double s, c;
    sincospi(-2.0 * (double)e / (double)g.N, &s, &c);
    rot = make_float2((float)c, (float)s);
  }
  uint64_t const kf = (uint64_t)f * (uint64_t)g.Lr;  // the frame's first k
  size_t const pz = (size_t)(kf % (uint64_t)g.Rz);
  uint64_t const per = 2 * (uint64_t)g.Fr;
  uint64_t const e0 = (2375 * (kf % per)) % per;
  double v[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < g.Lr; j += nthr) {
    float2 const z = kq::cmul(buf[g.skip + j], rot);
    size_t pos = pz + j;
    if (pos >= g.Rz) pos -= g.Rz;
    zr[pos] = z;
    double const zx = z.x, zy = z.y, p2 = zx * zx + zy * zy;
    uint64_t const e = (e0 + 2375 * (uint64_t)j) % per;  // (2375 k) mod 2 Fr
    double s, c;
    sincospi((double)e / (double)g.Fr, &s, &c);
    v[0] += zx * zx - zy * zy;
    v[1] += 2.0 * zx * zy;
    v[2] += p2 * c;
    v[3] -= p2 * s;
    v[4] += p2;
  }
  block_sums(v, red);
  if (tid == 0) {
    double *dst = a.sums + ((size_t)slot * g.Fmax + fi) * kSums;
#pragma unroll
    for (int c = 0; c < kSums; c++) dst[c] = v[c];
  }
}

__device__ __forceinline__ unsigned crc10(unsigned w) {  // remainder of w x^10 modulo x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
  unsigned r = (w & 0xFFFFu) << 10;
#pragma unroll
  for (int b = 25; b >= 10; b--)
    if ((r >> b) & 1u) r ^= 0x5B9u << (b - 10);
  return r & 0x3FFu;
}

// the position (0..3) of the offset word the syndrome equals, or -1; cp: it was C'
__device__ __forceinline__ int offset_pos(unsigned s, int &cp) {
  cp = s == 0x350u;
  return s == 0x0FCu ? 0 : s == 0x198u ? 1 : (s == 0x168u || s == 0x350u) ? 2 : s == 0x1B4u ? 3 : -1;
}

struct GroupOut {
  kq_rds_group *dst;   // the slot's row, or null
  unsigned cap, n;
};

__device__ __forceinline__ void put_word(RdsState &s, int pos, unsigned info) {
  s.blk = (s.blk & ~(0xFFFFull << (16 * pos))) | ((unsigned long long)(info & 0xFFFFu) << (16 * pos));
}
__device__ __forceinline__ void open_record(RdsState &s) {
  s.blk = 0;
  s.ok = s.vb = 0;
}
// (o.n < o.cap always holds: cap is max_groups() of the call, a bound on what a call can emit; the test keeps a store
// inside the row whatever happens)
__device__ __forceinline__ void emit(RdsState &s, GroupOut &o) {
  if (o.dst && o.n < o.cap) {
    kq_rds_group r;
    r.block[0] = (uint16_t)s.blk;
    r.block[1] = (uint16_t)(s.blk >> 16);
    r.block[2] = (uint16_t)(s.blk >> 32);
    r.block[3] = (uint16_t)(s.blk >> 48);
    r.ok = (uint8_t)s.ok;
    r.version_b = (uint8_t)s.vb;
    r.reserved = 0;
    r.bit = s.nbits;
    o.dst[o.n] = r;
  }
  if (o.n < o.cap) o.n++;
  open_record(s);
}

// one data bit through the block / group machine (the header's "Blocks", "Unsynced", "Synced")
__device__ __forceinline__ void push_bit(RdsState &s, unsigned b, int lose_after, GroupOut &o) {
  s.nbits++;
  s.reg = ((s.reg << 1) | b) & 0x3FFFFFFu;
  if (s.nbits < 26) return;
  unsigned const info = s.reg >> 10;
  int cp;
  int const pos = offset_pos(crc10(info) ^ (s.reg & 0x3FFu), cp);
  if (!s.synced) {
    if (pos < 0) return;
    if (s.rem_valid && s.nbits == s.rem_nbits + 26 && pos == ((s.rem_pos + 1) & 3)) {
      open_record(s);
      if (pos > 0) {
        put_word(s, s.rem_pos, s.rem_info);
        s.ok |= 1u << s.rem_pos;
        s.vb |= (unsigned)s.rem_cp;
        s.blocks_ok++;
      }
      put_word(s, pos, info);
      s.ok |= 1u << pos;
      s.vb |= (unsigned)cp;
      s.blocks_ok++;
      if (pos == 3) emit(s, o);
      s.synced = 1;
      s.expect = (pos + 1) & 3;
      s.next_at = s.nbits + 26;
      s.bad = 0;
    }
    s.rem_valid = 1;
    s.rem_nbits = s.nbits;
    s.rem_pos = pos;
    s.rem_info = info;
    s.rem_cp = cp;
    return;
  }
  if (s.nbits != s.next_at) return;
  int const want = s.expect;
  put_word(s, want, info);
  if (pos == want) {
    s.ok |= 1u << want;
    s.vb |= (unsigned)cp;
    s.blocks_ok++;
    s.bad = 0;
  } else {
    s.bad++;
    s.blocks_bad++;
  }
  if (want == 3) emit(s, o);
  s.expect = (want + 1) & 3;
  s.next_at += 26;
  if (s.bad >= lose_after) {
    s.synced = 0;
    s.rem_valid = 0;
    open_record(s);
  }
}

// one lane per slot: the call's frames in order
__global__ __launch_bounds__(64) void k_rds_track(CallArgs a, int nlist) {
  int const li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nlist) return;
  int const slot = a.list[li];
  RdsGeom const &g = a.g;
  RdsPar const p = a.par[slot];
  RdsState s = a.state[slot];
  const float2 *zr = a.z + (size_t)slot * g.Rz;
  GroupOut o;
  o.dst = a.groups ? a.groups + (size_t)slot * a.gstride : nullptr;
  o.cap = a.gcap;
  o.n = 0;
  double const two_pi = 2.0 * M_PI;
  for (int fi = 0; fi < a.F; fi++) {
    int64_t const f = (int64_t)(a.F0 + (uint64_t)fi);
    const double *sm = a.sums + ((size_t)slot * g.Fmax + fi) * kSums;
    s.ar += p.alpha * (sm[0] - s.ar);
    s.ai += p.alpha * (sm[1] - s.ai);
    s.br += p.alpha * (sm[2] - s.br);
    s.bi += p.alpha * (sm[3] - s.bi);
    double const w = atan2(s.ai, s.ar) - 2.0 * s.phi;
    s.phi += 0.5 * (w - two_pi * rint(w / two_pi));
    s.phi -= two_pi * ceil((s.phi - M_PI) / two_pi);  // into (-pi, pi]
    double const u = -atan2(s.bi, s.br) / two_pi - s.tau;
    s.tau += u - rint(u);
    double const lo = (double)f * g.Lr, hi = (double)(f + 1) * g.Lr;
    if (!s.started) {  // the least i with t_i >= f Lr
      long long i = (long long)ceil(lo / g.spb - s.tau);
      while (((double)i + s.tau) * g.spb < lo) i++;
      while (((double)(i - 1) + s.tau) * g.spb >= lo) i--;
      s.next_i = i;
      s.started = 1;
    }
    double rs, rc;
    sincos(s.phi, &rs, &rc);
    for (;;) {
      double const t = ((double)s.next_i + s.tau) * g.spb;
      if (!(t + 1.0 < hi)) break;
      double const fl = floor(t), r = t - fl;
      int64_t const k0 = (int64_t)fl;
      float2 const z0 = zr[ring_pos(k0, g.Rz)], z1 = zr[ring_pos(k0 + 1, g.Rz)];
      double const vx = (double)z0.x + r * ((double)z1.x - (double)z0.x), vy = (double)z0.y + r * ((double)z1.y - (double)z0.y);
      double const y = vx * rc + vy * rs;  // Re(v exp(-j phi))
      int const c = y < 0.0;
      push_bit(s, (unsigned)(c ^ s.cprev), p.lose_after, o);
      s.cprev = c;
      s.next_i++;
    }
    if (a.st) {
      kq_rds_status r;
      r.phase = (float)s.phi;
      r.timing = (float)s.tau;
      r.level = (float)sqrt(sm[4] / g.Lr);
      r.synced = s.synced;
      r.blocks_ok = s.blocks_ok;
      r.blocks_bad = s.blocks_bad;
      a.st[(size_t)slot * a.sstride + fi] = r;
    }
  }
  a.state[slot] = s;
  if (o.dst) {  // the rest of the slot's row reads as zeros, whatever an earlier call left there
    kq_rds_group zero{};
    for (unsigned k = o.n; k < o.cap; k++) o.dst[k] = zero;
  }
  if (a.counts) a.counts[slot] = o.n;
}

// H_r / N: the matched filter of the shaped biphase symbol (IEC 62106) round 57 kHz, one-sided
std::vector<float2> design_rds(int N, int M, double beta, double Fc) {
  std::vector<kq::cd> R((size_t)N, 0.0);
  double const td = 1.0 / kBitHz;
  for (int k = 0; k < N; k++) {
    double const gf = kq::bin_hz(k, N, Fc) - kSubHz;
    if (std::fabs(gf) <= 2.0 / td) R[k] = kq::cd(0.0, -1.0) * std::sin(M_PI * gf * td / 2) * std::cos(M_PI * gf * td / 4);
  }
  return kq::window_design(R, M, beta);
}

// The groups one call of nsamples can emit, at most.  Its frames F <= (nsamples + L - 1) / L cover F L <= nsamples + L - 1
// samples (up to L - 1 were carried in).  The bit sampler starts a call at an i with t_i + 1 >= the first frame's start under
// the tau before it and ends at one with t_i + 1 < the last frame's end under the last tau, and tau moves by at most half
// a bit per frame, so the call decodes fewer than F L 1187.5 / Fc + F / 2 + 1 bits; a group is emitted once per 104 bits
// counted, so at most floor(bits / 104) + 1 of them.  Never below ceil(nsamples 1187.5 / Fc) / 104 + 2.
size_t max_groups(int Fc, int L, size_t nsamples) {
  size_t const plain = (size_t)std::ceil((double)nsamples * kBitHz / Fc) / 104 + 2;
  size_t const F = (nsamples + (size_t)L - 1) / (size_t)L;
  double const bits = (double)(nsamples + (size_t)L - 1) * kBitHz / Fc + 0.5 * (double)F + 1.0;
  return std::max(plain, (size_t)std::floor(bits / 104.0) + 1);
}

}  // namespace

struct kq_rds_bank : kq::HostSide {
  kq_rds_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  RdsGeom g{};
  uint64_t n_cur = 0;
  uint64_t last_F0 = 0;                  // the last call's first frame and frame count (kq_rds_pull_baseband)
  int last_F = 0;
  size_t gmax = 0;                       // max_groups(max_samples)
  struct Dev {  // kq::lazy_device
    kq::SlotTable<RdsPar> slots;
    float *x = nullptr;
    float2 *z = nullptr;
    double *sums = nullptr;
    RdsState *state = nullptr;
    float2 *hr = nullptr;
    // host-memory calls
    kq_rds_group *groups = nullptr;
    uint32_t *counts = nullptr;
    kq_rds_status *st = nullptr;
  } d;
};

namespace {

int make_device(kq_rds_bank *b) {
  kq_rds_config const &c = b->cfg;
  RdsGeom &g = b->g;
  auto &d = b->d;
  bool okN = false, okR = false;
  g.dN = kq::fft_dim(g.N, &okN);
  g.dNr = kq::fft_dim(g.Nr, &okR);
  if (!okN || !okR) {
    kq_internal_set_error("kq_rds: no transform plan for N %d / N / Dr %d", g.N, g.Nr);
    return -1;
  }
  if (b->open_stream(c.stream)) return -1;
  size_t const S = c.max_slots;
  if (!(g.tw = kq::half_twiddles(kTwLog2))) {  // shared, not the bank's to free
    kq_internal_set_error("kq_rds: no twiddle table of period 2^%d", kTwLog2);
    return -1;
  }
  std::vector<float2> hr = design_rds(g.N, g.M, c.kaiser_beta, c.comp_rate);
  if (b->alloc(&d.hr, hr.size()) || d.slots.alloc(*b, S) || b->alloc(&d.x, S * g.Rx) || b->alloc(&d.z, S * g.Rz) ||
      b->alloc(&d.sums, S * g.Fmax * kSums) || b->alloc(&d.state, S, true))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.hr, hr.data(), hr.size() * sizeof(float2), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  g.hr = d.hr;
  return 0;
}

// zero history, zero tracker and machine (the stream is idle: callers synchronised it)
int cold_start(kq_rds_bank *b, unsigned s) {
  KQ_TRY(hipMemsetAsync(b->d.x + (size_t)s * b->g.Rx, 0, b->g.Rx * sizeof(float), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.z + (size_t)s * b->g.Rz, 0, b->g.Rz * sizeof(float2), b->stream));
  KQ_TRY(hipMemsetAsync(b->d.state + s, 0, sizeof(RdsState), b->stream));
  return 0;
}

}  // namespace

extern "C" {

kq_rds_bank *kq_rds_create(const kq_rds_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_rds_create: null config");
    return nullptr;
  }
  unsigned const Dr = cfg->decimate, L = cfg->L, M = cfg->M;
  if (cfg->comp_rate < 128000) {
    kq_internal_set_error("kq_rds_create: comp_rate %d must be >= 128000", cfg->comp_rate);
    return nullptr;
  }
  unsigned const Fc = (unsigned)cfg->comp_rate;
  if (Dr == 0 || Fc % Dr || Fc / Dr < 9500) {
    kq_internal_set_error("kq_rds_create: decimate %u must divide comp_rate %d and leave a rate of at least 9500", Dr,
                          cfg->comp_rate);
    return nullptr;
  }
  if (M < 3 || !(M & 1)) {
    kq_internal_set_error("kq_rds_create: M %u must be odd and >= 3", M);
    return nullptr;
  }
  if (L == 0 || L % Dr || (M - 1) % Dr) {
    kq_internal_set_error("kq_rds_create: decimate %u must divide L %u and M - 1 %u", Dr, L, M - 1);
    return nullptr;
  }
  unsigned long const N = (unsigned long)L + M - 1;
  if (N > (unsigned long)kMaxN || (N & 1) || !kq::fft_size_ok((int)N)) {
    kq_internal_set_error("kq_rds_create: N = L + M - 1 = %lu must be even, 2^a 3^b 5^c 7^d and <= %d", N, kMaxN);
    return nullptr;
  }
  if (((unsigned long long)kSubHz * N) % Fc) {
    kq_internal_set_error("kq_rds_create: 57000 N / comp_rate = 57000 x %lu / %d is not whole: the subcarrier must sit on a bin", N,
                          cfg->comp_rate);
    return nullptr;
  }
  if (!std::isfinite(cfg->kaiser_beta) || cfg->kaiser_beta < 0) {
    kq_internal_set_error("kq_rds_create: kaiser_beta must be finite and >= 0");
    return nullptr;
  }
  if ((double)(M - 1) / Fc < 3.0 / kBitHz) {
    kq_internal_set_error("kq_rds_create: M %u is shorter than three bit periods (M - 1 >= %.0f at comp_rate %d)", M,
                          std::ceil(3.0 * Fc / kBitHz), cfg->comp_rate);
    return nullptr;
  }
  double const trans = 2.0 * Fc * std::sqrt(1.0 + (double)cfg->kaiser_beta * cfg->kaiser_beta) / M;
  if (59375.0 + trans > Fc / 2.0) {
    kq_internal_set_error("kq_rds_create: 59375 Hz + transition band %.0f Hz does not fit below comp_rate / 2 (longer M, lower "
                          "kaiser_beta or a higher comp_rate)", trans);
    return nullptr;
  }
  if (cfg->max_slots == 0 || cfg->max_slots > kMaxSlots) {
    kq_internal_set_error("kq_rds_create: max_slots %u must be 1..%u", cfg->max_slots, kMaxSlots);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_rds_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  kq_rds_bank *b = new kq_rds_bank;
  b->cfg = *cfg;
  RdsGeom &g = b->g;
  g.N = (int)N;
  g.L = (int)L;
  g.M = (int)M;
  g.Dr = (int)Dr;
  g.Nr = (int)(N / Dr);
  g.Lr = (int)(L / Dr);
  g.skip = (int)((M - 1) / Dr);
  g.nthr = kq::fft_threads(g.N);
  g.Fmax = (int)((cfg->max_samples + L - 1) / L);
  g.Fc = (int)Fc;
  g.Fr = (int)(Fc / Dr);
  g.k0 = (int)(((unsigned long long)kSubHz * N) / Fc);
  g.spb = (double)g.Fr / kBitHz;
  g.Rx = cfg->max_samples + L - 1 + (M - 1);
  g.Rz = (size_t)g.Fmax * g.Lr + (size_t)std::ceil(g.spb) + 2;
  b->gmax = max_groups(g.Fc, g.L, cfg->max_samples);
  return b;
}

int kq_rds_destroy(kq_rds_bank *b) { return kq::destroy_bank(b, "kq_rds_destroy"); }

int kq_rds_set(kq_rds_bank *b, unsigned slot, const kq_rds_params *p) {
  if (!kq::set_args_ok("kq_rds_set", slot, p, kMaxSlots)) return -1;
  if (!std::isfinite(p->track_ms) || p->track_ms <= 0) {
    kq_internal_set_error("kq_rds_set: track_ms must be finite and positive");
    return -1;
  }
  if (p->lose_after < 1) {
    kq_internal_set_error("kq_rds_set: lose_after %d must be >= 1", p->lose_after);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_rds_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("kq_rds_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  RdsPar np{};
  np.active = 1;
  np.source = p->source;
  np.lose_after = p->lose_after;
  np.alpha = 1.0 - std::exp(-(double)b->g.L / ((double)b->g.Fc * (double)p->track_ms * 1e-3));
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_rds_remove(kq_rds_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_rds_remove"); }

size_t kq_rds_max_groups(const kq_rds_bank *b, size_t nsamples) {
  if (!b) {
    kq_internal_set_error("kq_rds_max_groups: null bank");
    return 0;
  }
  return max_groups(b->g.Fc, b->g.L, nsamples);
}

int kq_rds_process(kq_rds_bank *b, const float *comp, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_rds_group *groups, size_t groups_stride, uint32_t *counts,
                   kq_rds_status *status, size_t status_stride) {
  if (!b) {
    kq_internal_set_error("kq_rds_process: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::blocks_ok("kq_rds_process", b->cfg.max_samples, row_stride, block_len, nblocks)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  RdsGeom &g = b->g;
  uint64_t const n0 = b->n_cur, n1 = n0 + ncall, F0 = n0 / (uint64_t)g.L;
  int const F = (int)(n1 / (uint64_t)g.L - F0);
  size_t const gcall = max_groups(g.Fc, g.L, ncall);
  if (groups && groups_stride < gcall) {
    kq_internal_set_error("kq_rds_process: groups_stride %zu < kq_rds_max_groups = %zu", groups_stride, gcall);
    return -1;
  }
  if (status && status_stride < (size_t)F) {
    kq_internal_set_error("kq_rds_process: status_stride %zu < F = %d", status_stride, F);
    return -1;
  }
  kq::CallWork const work = kq::call_work(b, "kq_rds_process", ncall, comp, "comp");
  if (work == kq::CALL_IDLE) {
    b->n_cur = n1;
    b->last_F0 = F0;
    b->last_F = F;
    return F;
  }
  if (work != kq::CALL_RUN) return work;
  kq::DeviceScope dev_scope_(b->cfg.device);
  auto &d = b->d;
  size_t const S = b->cfg.max_slots, nlist = d.slots.all.size();
  CallArgs a{};
  a.g = g;
  a.par = d.slots.d_par;
  a.list = d.slots.d_list;
  a.x = d.x;
  a.z = d.z;
  a.sums = d.sums;
  a.state = d.state;
  a.n0 = n0;
  a.F0 = F0;
  a.F = F;
  a.block_len = block_len;
  a.xbase = (size_t)(n0 % (uint64_t)g.Rx);
  a.gcap = (unsigned)gcall;
  if (on_device) {
    a.comp = comp;
    a.src_stride = src_stride;
    a.row_stride = row_stride;
    a.rowmap = nullptr;
    a.groups = groups;
    a.gstride = groups_stride;
    a.counts = counts;
    a.st = status;
    a.sstride = status_stride;
  } else {
    kq::Staged in;
    if (d.slots.stage_rows(*b, comp, sizeof(float), src_stride, row_stride, block_len, nblocks,
                           b->cfg.max_samples * sizeof(float), &in))
      return -1;
    a.comp = static_cast<const float *>(in.src);
    a.src_stride = in.src_stride;
    a.row_stride = in.row_stride;
    a.rowmap = in.rowmap;
    if (groups && !d.groups && b->alloc(&d.groups, S * b->gmax)) return -1;
    if (counts && !d.counts && b->alloc(&d.counts, S)) return -1;
    if (status && !d.st && b->alloc(&d.st, S * (size_t)g.Fmax)) return -1;
    a.groups = groups ? d.groups : nullptr;
    a.gstride = b->gmax;
    a.counts = counts ? d.counts : nullptr;
    a.st = status ? d.st : nullptr;
    a.sstride = g.Fmax;
  }
  {
    unsigned const chunks = (unsigned)std::min<size_t>((ncall + 255) / 256, 1024);
    hipLaunchKernelGGL(k_rds_ingest, dim3(chunks, (unsigned)nlist), dim3(256), 0, b->stream, a, ncall);
    KQ_TRY(hipGetLastError());
  }
  if (F > 0) {
    size_t const lds = (size_t)g.N * sizeof(float2);
    kq::ensure_dynamic_lds((const void *)k_rds_front, lds);
    hipLaunchKernelGGL(k_rds_front, dim3((unsigned)F, (unsigned)nlist), dim3(g.nthr), lds, b->stream, a);
    KQ_TRY(hipGetLastError());
  }
  // (with no frame completed it still writes the counts: 0)
  hipLaunchKernelGGL(k_rds_track, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, b->stream, a, (int)nlist);
  KQ_TRY(hipGetLastError());
  if (!on_device) {
    // the rows of the active slots: groups and status when a frame was completed, the counts always
    auto back = [&](size_t s0, size_t n) {
      if (groups && F > 0 && kq::copy_rows_back(*b, groups, groups_stride, d.groups, a.gstride, gcall, sizeof(kq_rds_group), s0, n))
        return -1;
      if (counts) KQ_TRY(hipMemcpyAsync(counts + s0, d.counts + s0, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
      if (status && F > 0 && kq::copy_rows_back(*b, status, status_stride, d.st, a.sstride, (size_t)F, sizeof(kq_rds_status), s0, n))
        return -1;
      return 0;
    };
    if (d.slots.for_runs(back)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  b->n_cur = n1;  // only once everything is queued: a call that fails leaves the stream index where it was
  b->last_F0 = F0;
  b->last_F = F;
  return F;
}

int kq_rds_pull_baseband(kq_rds_bank *b, unsigned slot, float *dst_re_im, size_t cap_complex) {
  if (!b) {
    kq_internal_set_error("kq_rds_pull_baseband: null bank");
    return -1;
  }
  if (!dst_re_im) {
    kq_internal_set_error("kq_rds_pull_baseband: null dst_re_im");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->d.slots.active(slot)) {
    kq_internal_set_error("kq_rds_pull_baseband: slot %u holds no decoder", slot);
    return -1;
  }
  RdsGeom const &g = b->g;
  size_t const n = std::min((size_t)b->last_F * g.Lr, cap_complex);
  if (n == 0) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  const float2 *zr = b->d.z + (size_t)slot * g.Rz;
  size_t const p0 = (size_t)((b->last_F0 * (uint64_t)g.Lr) % (uint64_t)g.Rz), first = std::min(n, g.Rz - p0);
  KQ_TRY(hipMemcpyAsync(dst_re_im, zr + p0, first * sizeof(float2), hipMemcpyDeviceToHost, b->stream));
  if (n > first)
    KQ_TRY(hipMemcpyAsync(dst_re_im + 2 * first, zr, (n - first) * sizeof(float2), hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return (int)n;
}

int kq_rds_sync(kq_rds_bank *b) { return kq::sync_bank(b, "kq_rds_sync"); }

int kq_rds_reset(kq_rds_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_rds_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  b->last_F0 = 0;
  b->last_F = 0;
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  for (int s : b->d.slots.all)
    if (cold_start(b, (unsigned)s)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // extern "C"
