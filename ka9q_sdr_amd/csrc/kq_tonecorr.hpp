// kq_tonecorr.hpp -- what the banks that correlate PCM against tones from a cosine table share (kq_tone: DTMF and selective
// calling; kq_cw: Morse; kq_rtty: start-stop FSK; kq_psk: PSK31; kq_ale: ALE 8-FSK), and the quantiser that the FSK front end (kq_fskfront.hpp) shares with them.
//
//   load_q           the header's quantiser (include/ka9q_hip.h, kq_fsk_*): sample i of a call, f32 or s16be, over kq::PcmIn
//   cos_table        C[j] = rint(32767 cos(2 pi j / 1024)), one instance for the library; get_table, the body of
//                    kq_*_get_table; load_packed_table, cosine and sine of an entry in one LDS word
//   FrameGrid        kq_cw, kq_rtty, kq_psk and kq_ale: frames of B samples on a grid that starts at sample 0 of the stream, each at a stride
//                    Bs >= B in LDS with Bs / 2 odd, so that lanes reading sample i of 32 consecutive frames hit 32 banks; the
//                    choice of L, the lanes to a frame, per bank (least_lanes) and per call (lanes_for_call)
//   correlate_piece  the front half of k_cw's, k_rtty's, k_psk's and k_ale's piece loop: 64 / L frames through LDS, NT tones each
//
// What a bank does with the sums -- its tracker, its history, its events -- stays with the bank, and so does k_tone, which
// has another shape (a workgroup per slot, many tones).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ka9q_hip.h"
#include "kq_host.hpp"
#include "kq_slots.hpp"

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

constexpr int kTable = 1024;

// made once, at the first kq_*_create of any of the banks
inline std::vector<short> const &cos_table() {
  static std::vector<short> const table = [] {
    std::vector<short> t((size_t)kTable);
    for (int j = 0; j < kTable; j++) t[j] = (short)std::lrint(32767.0 * std::cos(2.0 * M_PI * j / kTable));
    return t;
  }();
  return table;
}

// the table on the device (queued: the caller waits)
inline int alloc_table(HostSide &h, short **table) {
  if (h.alloc(table, (size_t)kTable)) return -1;
  KQ_TRY(hipMemcpyAsync(*table, cos_table().data(), kTable * sizeof(short), hipMemcpyHostToDevice, h.stream));
  return 0;
}

// kq_*_get_table
inline int get_table(const void *b, const char *fn, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("%s: null dst", fn);
    return -1;
  }
  size_t const n = std::min(cap, (size_t)kTable);
  if (n) std::memcpy(dst, cos_table().data(), n * sizeof(int16_t));
  return kTable;
}

// CS[j]: C[j] in the low half, C[(j - 256) & 1023] in the high (the caller's next barrier makes it visible)
__device__ __forceinline__ void load_packed_table(int *CS, const short *table, int tid, int nthreads) {
  for (int i = tid; i < kTable; i += nthreads) CS[i] = ((int)table[i] & 0xFFFF) | ((int)table[(i - 256) & (kTable - 1)] << 16);
}

struct FrameGrid {
  int B, Bs;       // Bs: a frame's stride in LDS, >= B, Bs / 2 odd
  unsigned magic;  // ceil(2^32 / B): x / B = umulhi(x, magic) for x < 2^16
};

inline FrameGrid frame_grid(unsigned block_len) {
  FrameGrid g;
  g.B = (int)block_len;
  g.Bs = g.B + ((g.B & 1) ? 1 : 0);  // even
  if ((g.Bs & 3) == 0) g.Bs += 2;    // and Bs / 2 odd
  g.magic = (unsigned)((0x100000000ull + block_len - 1) / block_len);
  return g;
}

// the least lanes to a frame with which a piece, 64 / L frames, fits `tile` samples of LDS (64 at the latest where Bs <= tile)
inline int least_lanes(FrameGrid const &g, int tile) {
  int L = 1;
  while ((64 / L) * g.Bs > tile) L *= 2;
  return L;
}

// lanes to a frame for a call of ncall samples: what the piece needs, and more where the call's frames (at most nf) do not
// fill a wave.  The sums are exact, so L changes no result.
inline int lanes_for_call(FrameGrid const &g, int Lmin, size_t ncall) {
  size_t const nf = (ncall + (size_t)g.B - 2) / (size_t)g.B + 1;
  int L = Lmin;
  while (L < 64 && (size_t)(2 * L) * nf <= 64) L *= 2;
  return L;
}

// One piece of a wave's slot: the frames k0 .. k0 + 64 / L - 1 of the grid, of which the call (samples n0 ..) has x0 .. x1 - 1,
// counted from k0 B; n is the stream index of x0.  The samples go into q, quantised, each frame at stride Bs; lane (f, p) of
// 64 / L x L takes samples p, p + L, ... of frame f against the NT tones with phase increments inc[] -- one sample read, NT
// packed table reads, 2 NT 64-bit multiply-adds; the phase is a function of the sample index alone.  The L partial sums
// of a frame are folded by shuffles into sm[2 t], sm[2 t + 1] (I, Q of tone t; the frame's leader p == 0 has them), and lane
// 0 adds and clears the carried sums cy[] of the frame the call before ended in.  Every wave of the workgroup calls it, live
// or not: it begins with the barrier that ends the piece before (and, at the first piece, makes CS visible), and has one more
// between the load and the correlation.
template <int NT>
__device__ __forceinline__ void correlate_piece(FrameGrid const &g, PcmIn const &in, size_t row, bool live, int lane, int L,
                                                int64_t n0, int64_t n, int64_t k0, int x0, int x1, short *q, const int *CS,
                                                const unsigned (&inc)[NT], long long (&sm)[2 * NT], long long (&cy)[2 * NT]) {
  int const B = g.B, f = lane / L, p = lane & (L - 1);
  __syncthreads();
  if (live) {
    for (int x = x0 + lane; x < x1; x += 64) {
      unsigned const fr = __umulhi((unsigned)x, g.magic);
      q[fr * g.Bs + ((unsigned)x - fr * (unsigned)B)] = (short)load_q(in, row, (unsigned)(n - n0) + (unsigned)(x - x0));
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 2 * NT; t++) sm[t] = 0;
  int const xa = x0 > f * B ? x0 : f * B, xb = x1 < (f + 1) * B ? x1 : (f + 1) * B;
  if (live) {
    unsigned const at = (unsigned)(k0 * B) + (unsigned)(xa + p);  // (n inc) mod 2^32 needs n mod 2^32 only
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

}  // namespace tonecorr
}  // namespace kq
