// kq_bitclock.hpp -- the kernel of the two-tone banks with a bit clock (kq_dsc, kq_navtex, kq_same), written once: a
// frame-grid kernel with a window and a symbol clock, on top of kq_tonecorr.hpp, which describes the mapping.
//
// bit_clock<T, Args>   One wave per slot, four slots to a workgroup.  Two tones, four series, as k_rtty: every frame of B
//         samples against the mark and the space tone; lane f sums its own W entries per series and squares; lane 0 walks
//         the piece's (Pm, Ps) pairs in order through the three-point clock -- it reads LDS at the points only -- and at
//         every third point, the late one, hands the bit to the bank's tracker T.  The kernel itself is the template and
//         takes its arguments by value: a named kernel around a force-inlined body compiled to another register allocation
//         and schedule, which is the state in which the window block as a helper was measured slower
//         (profiles/r11/README.md).  The three instances compile to the listings the banks had as kernels of their own,
//         instruction for instruction (profiles/r12/README.md, which also says what that took).
//
// T, the tracker above the bit.  A kernel trace tells the instances apart by its name: k_dsc, k_navtex, k_same.
//   Geom, Status, Event   the bank's geometry (GridArgs::g), the slot's carried record, its events
//   Side                  what the tracker keeps in LDS per wave between load and store, lane 0 alone touching it (kq_dsc's
//                         open message, kq_same's tally); NoSide where it keeps nothing, which costs no LDS
//   load(c, w, s, side, nev), store(c, w, s, side, nev)   every lane: the record into lane 0 (s, nev) and back; load
//                         returns the slot's arena.  They get the workgroup's whole side[] and index it by w.wave
//                         themselves: an address formed at the call moves the listing of a tracker that has no use for
//                         it there.  WholeRecord: the two for a record that travels whole through lane 0
//   bit_step(g, par, s, side, pl, k, ev, nev)             lane 0: the late point of a bit at frame k, with the late power pl
//   kParks                true: the record is too long for lane 0's registers, and what a bit seldom touches waits in LDS
//                         from the load to the store: the window sums of the last completed frame in lastsum, and in Side
//                         what park(s, side, wave) puts there and unpark(s, side, wave) takes back (lane 0).  false:
//                         the sums go into s.sum after every piece that completes a frame
// Steps 1 and 2 of a bit are tc::bit_levels.  The head of the trackers' file() functions (the event counted, the arena full)
// stays written out in each: as one function it moved all three listings.
#pragma once
#include "kq_tonecorr.hpp"

namespace kq {
namespace bitclock {

namespace tc = kq::tonecorr;
using tc::kHist;
using tc::kTable;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 3200;                     // samples a wave keeps in LDS: 64 frames of B = 48 at stride 50; with the rest
                                                // the workgroup stays under 40 KiB, four workgroups to a CU
constexpr int kRow = kHist + 64 + 1;            // a wave's reduced sums of one kind: the history and a piece's frames

struct NoSide {};  // T::Side of a tracker that keeps nothing in LDS: never referenced, so the array takes none

// T::load and T::store of a tracker whose record travels whole through lane 0
struct WholeRecord {
  template <class Args, class Place, class Status, class Sides>
  static __device__ __forceinline__ auto load(Args const &c, Place const &w, Status &s, Sides &, unsigned &nev) {
    return tc::load_record(c, w, s, nev);
  }
  template <class Args, class Place, class Status, class Sides>
  static __device__ __forceinline__ void store(Args const &c, Place const &w, Status const &s, Sides &, unsigned nev) {
    tc::store_record(c, w, s, nev);
  }
};

// (four waves to a SIMD asked for: left to itself the allocator takes more VGPRs than the 128 that four workgroups to a CU
// allow; with the bound k_dsc takes 123 and no scratch)
template <class T, class Args>
__global__ __launch_bounds__(kThreads, 4) void bit_clock(Args c) {
  __shared__ int CS[kTable];                       // C[j] in the low half, C[(j - 256) & 1023] in the high
  __shared__ short qs[kWaves][kTile];
  __shared__ int A[kWaves][4][kRow];               // reduced sums: [0, kHist) the frames before the piece, then the piece's
  __shared__ unsigned long long Pb[kWaves][2][64];
  __shared__ long long carry[kWaves][4];
  __shared__ int lastsum[kWaves][4];
  __shared__ typename T::Side side[kWaves];        // between the record's load and its store lane 0 alone has it
  typename T::Geom const &g = c.g;
  auto const w = tc::wave_place<kThreads>(c, CS);
  int const wave = w.wave, lane = w.lane, W = tc::window_frames(w.live, w.par.W);
  unsigned const inc[2] = {w.par.inc_m, w.par.inc_s};
  int const q = w.par.tb >> 2;
  typename T::Status s{};
  unsigned nev = 0;
  typename T::Event *ev = T::load(c, w, s, side, nev);  // (the first barrier of correlate_piece is behind it)
  tc::load_hist(A[wave], c.hist, w);
  long long cy[4] = {s.acc[0][0], s.acc[0][1], s.acc[1][0], s.acc[1][1]};
  if constexpr (T::kParks)      // (a piece without a completed frame leaves lastsum alone, and its other writers stand
    if (w.live && lane == 0) {  // behind the first barrier below)
      T::park(s, side, wave);
      lastsum[wave][0] = s.sum[0][0];
      lastsum[wave][1] = s.sum[0][1];
      lastsum[wave][2] = s.sum[1][0];
      lastsum[wave][3] = s.sum[1][1];
    }
  for (tc::Piece pc(c.n0, w.B); pc.n < c.n1; pc.next(w.F)) {
    pc.span(c.n1, w.B, w.F);
    long long sm[4];  // (its first barrier: the piece before is done with q, A, Pb, carry and lastsum, and A is loaded)
    tc::correlate_piece<2>(c, w, pc, qs[wave], CS, inc, sm, cy);
    int const done = pc.done(g.grid);
    tc::file_sums(A[wave], carry[wave], w, pc, done, sm, 12);
    __syncthreads();
    int keep[4] = {0, 0, 0, 0};
    if (lane < done) {
      int v[4] = {0, 0, 0, 0};  // the window that ends at frame `lane`: W entries, the last at kHist + lane; the four series
      for (int i = 0; i < W; i++)  // side by side, as k_rtty has them
        for (int t = 0; t < 4; t++) v[t] += A[wave][t][kHist + lane - i];
      Pb[wave][0][lane] = (unsigned long long)((long long)v[0] * v[0]) + (unsigned long long)((long long)v[1] * v[1]);
      Pb[wave][1][lane] = (unsigned long long)((long long)v[2] * v[2]) + (unsigned long long)((long long)v[3] * v[3]);
      if (lane == done - 1)
        for (int t = 0; t < 4; t++) lastsum[wave][t] = v[t];
    }
    tc::keep_hist(A[wave], lane, done, keep);
    __syncthreads();
    tc::put_hist(A[wave], lane, keep);
    if (w.live && lane == 0) {
      for (int i = 0; i < done; i++) {  // the header's step, frame k0 + i
        s.frames = tc::sat_inc(s.frames);
        s.t -= 256;
        if (s.t >= 128) continue;
        unsigned long long const Pm = Pb[wave][0][i], Ps = Pb[wave][1][i], hi = Pm >= Ps ? Pm : Ps, lo = Pm >= Ps ? Ps : Pm;
        if (s.ph == 0) {
          s.pe = hi;
          s.t += q;
          s.ph = 1;
        } else if (s.ph == 1) {
          s.bit = Pm >= Ps ? 1u : 0u;
          s.hi = hi;
          s.lo = lo;
          s.t += q;
          s.ph = 2;
        } else {
          s.ph = 0;
          T::bit_step(g, w.par, s, side[wave], hi, (unsigned long long)(pc.k0 + i), ev, nev);
        }
      }
      if constexpr (!T::kParks)
        if (done) {
          s.sum[0][0] = lastsum[wave][0];
          s.sum[0][1] = lastsum[wave][1];
          s.sum[1][0] = lastsum[wave][2];
          s.sum[1][1] = lastsum[wave][3];
        }
      tc::take_carry(carry[wave], w, pc, done, cy);
    }
  }
  __syncthreads();
  tc::store_hist(A[wave], c.hist, w);
  if constexpr (T::kParks)
    if (w.live && lane == 0) {
      T::unpark(s, side, wave);
      s.sum[0][0] = lastsum[wave][0];
      s.sum[0][1] = lastsum[wave][1];
      s.sum[1][0] = lastsum[wave][2];
      s.sum[1][1] = lastsum[wave][3];
    }
  s.acc[0][0] = cy[0];
  s.acc[0][1] = cy[1];
  s.acc[1][0] = cy[2];
  s.acc[1][1] = cy[3];
  T::store(c, w, s, side, nev);  // (behind the barrier above)
}

}  // namespace bitclock
}  // namespace kq
