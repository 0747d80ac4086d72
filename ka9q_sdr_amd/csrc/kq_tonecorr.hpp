// kq_tonecorr.hpp -- the device half of what the banks that correlate PCM against tones from a cosine table share.  The
// host half (the table itself, the frame grid, the frame-grid banks' host bodies) is kq_gridbank.hpp, included here.
//
//   every user       (kq_tone, kq_cw, kq_rtty, kq_psk, kq_acars, kq_ale, and kq_bitclock.hpp for kq_dsc, kq_navtex and
//                     kq_same; load_q also kq_fskfront.hpp, for kq_fsk and kq_pag)
//     load_q             the header's quantiser (include/ka9q_hip.h, kq_fsk_*): sample i of a call, f32 or s16be, over kq::PcmIn
//     load_packed_table  cosine and sine of a table entry in one LDS word
//     sat_inc, mag, smooth, gate16   the counters, |v|, the one-pole levels and the 128-bit gate 16 sig >= snr nse
//   frame-grid banks (kq_cw, kq_rtty, kq_psk, kq_ale, kq_bitclock.hpp)
//     Place, wave_place  where a wave stands: its slot, its row of the input, its lanes' frame and place in it
//     load_record, store_record   the slot's carried record and event count, into lane 0 and back
//     Piece              the piece loop's bookkeeping
//     correlate_piece    the front half of the piece loop: 64 / L frames through LDS, NT tones each
//     take_carry         the sums of the frame a call ends in, back to lane 0
//   ... with a window (kq_rtty, kq_psk, kq_ale, kq_bitclock.hpp)
//     window_frames, load_hist, file_sums, keep_hist, put_hist, store_hist   the carried history of 31 frames in front of
//                        a piece's reduced sums (k_psk keeps the load and the store written out: measured slower there)
//     window_sum         the window slid over both, a series at a time: k_ale alone calls it (k_rtty and k_psk sum their
//                        four and two series side by side in one loop, which measured faster there)
//   ... with a symbol clock (kq_psk, kq_ale, kq_bitclock.hpp)
//     clock_adjust       the timing update of a symbol's step 1 (the three-point walk stays in the kernels: see there)
//     bit_levels         steps 1 and 2 of a bit of kq_bitclock.hpp's trackers (k_dsc, k_navtex, k_same)
//
// The frame-grid kernels, written once.  One wave per slot, four slots to a workgroup: a slot has a few tones and frames of
// a few dozen samples, so a workgroup per slot (k_tone) would leave most of its lanes without work.  The call's samples go
// through LDS once, a piece of 64 / L frames at a time, quantised as they are loaded (coalesced: lane i takes samples i,
// i + 64, ...), each frame at a stride Bs >= B with Bs / 2 odd.  Lane (f, p) of 64 / L x L takes samples p, p + L, ... of
// frame f and uses each for every tone: one sample read, NT packed table reads, 2 NT 64-bit multiply-adds; its phase comes
// from the sample index.  L = 1 where 64 frames fit the piece and the call has that many: then no lane talks to another.
// Otherwise the L partial sums of a frame are folded by shuffles; the sums are exact, so L changes no result, and the host
// picks it per call.  With a window, the frame leaders write the reduced sums to LDS behind the 31 carried frames of
// history (W <= 32) and the window is summed from there -- exact, so no scan order matters.  Lane 0 then walks the piece's
// completed frames in order through the bank's tracker, with the carried record in its registers; the other waves of the
// workgroup meet it at the next barrier.  The baud rate and W differ from slot to slot; B and the frame grid are the
// bank's, so every wave of a workgroup has the same pieces and the barriers are uniform.  The carried record and the
// history are read once and written once per call.  No atomics, no scratch.
//
// Everything here is force-inlined, takes the kernel's own __shared__ arrays and allocates none: a kernel's LDS is declared
// in the kernel, and so are its barriers.  What a bank does with the sums -- its tracker, its events, what it takes at a
// symbol's centre -- stays with the bank, and so do k_tone and k_acars, which have other shapes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "ka9q_hip.h"
#include "kq_gridbank.hpp"

namespace kq {

// q of the call's i-th sample (i < 2^28: max_samples)
__device__ __forceinline__ int load_q(PcmIn const &a, size_t row, unsigned i) {
  unsigned const k = i / a.block_len, j = i - k * a.block_len;
  size_t const idx = row * a.src_stride + (size_t)k * a.row_stride + j;
  if (a.format == KQ_PCM_S16BE) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a.src) + 2 * idx;
    int const w = (int)(short)(unsigned short)(((unsigned)p[0] << 8) | p[1]);
    return w < -32767 ? -32767 : w;
  }
  float const v = rintf(reinterpret_cast<const float *>(a.src)[idx] * a.scale);
  if (!(v == v)) return 0;
  return (int)fminf(fmaxf(v, -32767.f), 32767.f);
}

namespace tonecorr {

// CS[j]: C[j] in the low half, C[(j - 256) & 1023] in the high (the caller's next barrier makes it visible)
__device__ __forceinline__ void load_packed_table(int *CS, const short *table, int tid, int nthreads) {
  for (int i = tid; i < kTable; i += nthreads) CS[i] = ((int)table[i] & 0xFFFF) | ((int)table[(i - 256) & (kTable - 1)] << 16);
}

__device__ __forceinline__ unsigned sat_inc(unsigned v) { return v == 0xFFFFFFFFu ? v : v + 1; }

__device__ __forceinline__ long long mag(long long v) { return v < 0 ? -v : v; }

// v += (x - v) >> sh: both below 2^63, so the difference fits
__device__ __forceinline__ void smooth(uint64_t &v, uint64_t x, int sh) {
  v = (uint64_t)((long long)v + (((long long)x - (long long)v) >> sh));
}

// 16 sig >= snr nse in 128 bits: (sig >> 60, sig << 4) against (umulhi(nse, snr), nse snr)
__device__ __forceinline__ bool gate16(uint64_t sig, uint64_t nse, unsigned snr) {
  unsigned long long const lh = sig >> 60, ll = sig << 4, rh = __umul64hi(nse, (unsigned long long)snr),
                           rl = nse * (unsigned long long)snr;
  return lh > rh || (lh == rh && ll >= rl);
}

// ---- the frame-grid kernels ------------------------------------------------------------------------------------------
template <class Par>
struct Place {
  int wave, lane, slot;  // slot 0 where the wave has none (live false): it goes through the barriers with the others
  bool live;
  Par par;
  size_t row;            // of the call's input
  int B, L, F, f, p;     // F = 64 / L frames to a piece; the lane is p of frame f's L
};

// c: the kernel's argument block (GridArgs); also loads CS, which the first barrier of correlate_piece makes visible
template <int NTHREADS, class Args>
__device__ __forceinline__ auto wave_place(Args const &c, int *CS) {
  Place<typename std::remove_cv<typename std::remove_pointer<decltype(c.par)>::type>::type> w;
  int const tid = threadIdx.x, li = (int)blockIdx.x * (NTHREADS / 64) + (tid >> 6);
  w.wave = tid >> 6;
  w.lane = tid & 63;
  w.live = li < c.nlist;
  w.slot = w.live ? c.list[li] : 0;
  load_packed_table(CS, c.table, tid, NTHREADS);
  w.par = c.par[w.slot];
  w.row = w.live && c.rowmap ? (size_t)c.rowmap[li] : (size_t)w.par.source;
  w.B = c.g.grid.B;
  w.L = c.L;
  w.F = 64 / w.L;
  w.f = w.lane / w.L;
  w.p = w.lane & (w.L - 1);
  return w;
}

// carried: lane 0 holds the record, the open frame's sums in it; returns the slot's arena
template <class Args, class Par, class Status>
__device__ __forceinline__ auto load_record(Args const &c, Place<Par> const &w, Status &s, unsigned &nev) {
  if (w.live && w.lane == 0) {
    s = c.state[w.slot];
    nev = c.nev[w.slot];
  }
  return c.ev + (size_t)w.slot * c.g.max_events;
}

template <class Args, class Par, class Status>
__device__ __forceinline__ void store_record(Args const &c, Place<Par> const &w, Status const &s, unsigned nev) {
  if (w.live && w.lane == 0) {
    c.state[w.slot] = s;
    c.nev[w.slot] = nev;
    if (c.st) c.st[(size_t)w.slot * c.sstride] = s;
  }
}

// One piece: the frames k0 .. k0 + F - 1 of the grid, from n, the stream index of x0, to their end or the call's at n1.
// x counts from k0 B: the call has x0 .. x1 - 1 of the piece, x1 <= F B.
//   for (Piece pc(c.n0, B); pc.n < c.n1; pc.next(F)) { pc.span(c.n1, B, F); ... }
struct Piece {
  int64_t n, k0, e;  // e: where the piece ends
  int x0, x1;
  __device__ __forceinline__ Piece(int64_t n0, int B) : n(n0), k0(n0 / B), e(n0), x0(0), x1(0) {}
  __device__ __forceinline__ void span(int64_t n1, int B, int F) {
    int64_t const pe = (k0 + F) * (int64_t)B;
    e = pe < n1 ? pe : n1;
    x0 = (int)(n - k0 * B);
    x1 = x0 + (int)(e - n);
  }
  __device__ __forceinline__ int done(FrameGrid const &g) const { return (int)__umulhi((unsigned)x1, g.magic); }  // complete frames
  __device__ __forceinline__ void next(int F) {
    n = e;
    k0 += F;
  }
};

// The samples of piece pc go into q, quantised, each frame at stride Bs; lane (f, p) of 64 / L x L takes samples p, p + L,
// ... of frame f against the NT tones with phase increments inc[]; the phase is a function of the sample index alone.  The
// L partial sums of a frame are folded by shuffles into sm[2 t], sm[2 t + 1] (I, Q of tone t; the frame's leader p == 0 has
// them), and lane 0 adds and clears the carried sums cy[] of the frame the call before ended in.  Every wave of the
// workgroup calls it, live or not: it begins with the barrier that ends the piece before (and, at the first piece, makes CS
// visible), and has one more between the load and the correlation.
template <int NT, class Args, class Par>
__device__ __forceinline__ void correlate_piece(Args const &c, Place<Par> const &w, Piece const &pc, short *q, const int *CS,
                                                const unsigned (&inc)[NT], long long (&sm)[2 * NT], long long (&cy)[2 * NT]) {
  FrameGrid const &g = c.g.grid;
  int const B = g.B, f = w.f, p = w.p, L = w.L, lane = w.lane, x0 = pc.x0, x1 = pc.x1;
  __syncthreads();
  if (w.live) {
    for (int x = x0 + lane; x < x1; x += 64) {
      unsigned const fr = __umulhi((unsigned)x, g.magic);
      q[fr * g.Bs + ((unsigned)x - fr * (unsigned)B)] = (short)load_q(c.in, w.row, (unsigned)(pc.n - c.n0) + (unsigned)(x - x0));
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2 * NT; t++) sm[t] = 0;
  int const xa = x0 > f * B ? x0 : f * B, xb = x1 < (f + 1) * B ? x1 : (f + 1) * B;
  if (w.live) {
    unsigned const at = (unsigned)(pc.k0 * B) + (unsigned)(xa + p);  // (n inc) mod 2^32 needs n mod 2^32 only
    unsigned ph[NT], step[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      ph[t] = at * inc[t];
      step[t] = (unsigned)L * inc[t];
    }
    const short *qf = q + f * (g.Bs - B);
    for (int x = xa + p; x < xb; x += L) {
      int const v = qf[x];
      int cs[NT];
#pragma unroll
      for (int t = 0; t < NT; t++) cs[t] = CS[ph[t] >> 22];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        sm[2 * t] += (long long)v * (short)cs[t];
        sm[2 * t + 1] += (long long)v * (cs[t] >> 16);
        ph[t] += step[t];
      }
    }
  }
  for (int off = L >> 1; off; off >>= 1)
#pragma unroll
    for (int t = 0; t < 2 * NT; t++) sm[t] += __shfl_xor(sm[t], off);
  if (lane == 0)  // frame 0 of the call's first piece goes on from the carried sums
#pragma unroll
    for (int t = 0; t < 2 * NT; t++) {
      sm[t] += cy[t];
      cy[t] = 0;
    }
}

// lane 0, behind the barrier that follows the frame leaders' writes: where the call ends inside frame `done`, that frame's
// sums, which its leader left in carry[], for the next call
template <int NS, class Par>
__device__ __forceinline__ void take_carry(const long long (&carry)[NS], Place<Par> const &w, Piece const &pc, int done,
                                           long long (&cy)[NS]) {
  if (done * w.B < pc.x1)
#pragma unroll
    for (int t = 0; t < NS; t++) cy[t] = carry[t];
}

// ---- the history window ----------------------------------------------------------------------------------------------
// A: a wave's reduced sums, a series to a row of ROW >= kHist + 64 words: [0, kHist) the frames before the piece, then the
// piece's.  (The host keeps W in 8..32.)
__device__ __forceinline__ int window_frames(bool live, int W) { return live ? min(max(W, 1), kHist + 1) : 1; }

// the history to the front of A (the first barrier of correlate_piece makes it visible)
template <int NS, int ROW, class Par>
__device__ __forceinline__ void load_hist(int (&A)[NS][ROW], const FrameHist<NS> *hist, Place<Par> const &w) {
  if (w.lane < kHist)
    for (int t = 0; t < NS; t++) A[t][w.lane] = w.live ? hist[w.slot].v[t][w.lane] : 0;
}

// the frame leaders: the sums of a complete frame, reduced, behind the history; those of the frame the call ends in to carry
template <int NS, int ROW, class Par>
__device__ __forceinline__ void file_sums(int (&A)[NS][ROW], long long (&carry)[NS], Place<Par> const &w, Piece const &pc, int done,
                                          const long long (&sm)[NS], int shift) {
  if (w.p == 0 && w.f * w.B < pc.x1) {
    if (w.f < done) {
#pragma unroll
      for (int t = 0; t < NS; t++) A[t][kHist + w.f] = (int)(sm[t] >> shift);
    } else {
#pragma unroll
      for (int t = 0; t < NS; t++) carry[t] = sm[t];
    }
  }
}

// the window of one series that ends at frame `fr` of the piece: W entries, the last at kHist + fr
__device__ __forceinline__ int window_sum(const int *series, int fr, int W) {
  int w = 0;
  for (int i = 0; i < W; i++) w += series[kHist + fr - i];
  return w;
}

// what the next piece finds in front, the last kHist frames: out of A before a barrier, and back behind it
template <int NS, int ROW>
__device__ __forceinline__ void keep_hist(int (&A)[NS][ROW], int lane, int done, int (&keep)[NS]) {
  if (lane < kHist)
#pragma unroll
    for (int t = 0; t < NS; t++) keep[t] = A[t][done + lane];
}

template <int NS, int ROW>
__device__ __forceinline__ void put_hist(int (&A)[NS][ROW], int lane, const int (&keep)[NS]) {
  if (lane < kHist)
#pragma unroll
    for (int t = 0; t < NS; t++) A[t][lane] = keep[t];
}

// at the end of the call, behind a barrier
template <int NS, int ROW, class Par>
__device__ __forceinline__ void store_hist(const int (&A)[NS][ROW], FrameHist<NS> *hist, Place<Par> const &w) {
  if (w.live && w.lane < kHist)
    for (int t = 0; t < NS; t++) hist[w.slot].v[t][w.lane] = A[t][w.lane];
}

// ---- the symbol clock ------------------------------------------------------------------------------------------------
// The status record names t, pe, ee and el.  The three-point walk itself (s.t -= 256; if (s.t >= 128) continue; then the
// early, the centre or the late point by s.ph) stays written out in k_psk and k_ale: as a function that answers which point
// a frame hit it cost k_psk 9 % and k_ale 1 to 2 % at 4096-sample calls on the MI355X, whether it took the power by
// reference or through a callable (and its first form, two branches that stored through one selected address, put 24
// bytes of the record in scratch).
//
// step 1 of a symbol, at its late point with the late power pl: the early and the late level, and the next early point
template <class Status>
__device__ __forceinline__ void clock_adjust(Status &s, int tb, unsigned long long pl) {
  smooth(s.ee, s.pe, 3);
  smooth(s.el, pl, 3);
  unsigned long long const m = s.ee > s.el ? s.ee : s.el;
  int adj = 0;
  if (s.ee > s.el && s.ee - s.el > (m >> 3)) adj = -(tb >> 5);
  else if (s.el > s.ee && s.el - s.ee > (m >> 3)) adj = tb >> 5;
  s.t += tb - 2 * (tb >> 2) + adj;
}

// steps 1 and 2 of a bit of the two-tone banks (kq_bitclock.hpp), at its late point with the late power pl: the timing with
// the centre level, the signal and the noise level; answers whether the gate is open
template <class Geom, class Par, class Status>
__device__ __forceinline__ bool bit_levels(Geom const &g, Par const &par, Status &s, unsigned long long pl) {
  // 1 timing
  clock_adjust(s, par.tb, pl);
  smooth(s.ec, s.hi, 3);
  unsigned long long const top = s.ee > s.el ? s.ee : s.el, low = s.ee > s.el ? s.el : s.ee;
  if (top - low <= (top >> 3) && s.ec + (top >> 3) < low) s.t += par.tb >> 5;  // (adj == 0) half a bit out: no slope there
  // 2 levels and gate
  smooth(s.sig, s.hi, 4);
  smooth(s.nse, s.lo, 4);
  return s.frames >= g.warm && s.sig >= g.min_p && gate16(s.sig, s.nse, g.snr);
}

}  // namespace tonecorr
}  // namespace kq
