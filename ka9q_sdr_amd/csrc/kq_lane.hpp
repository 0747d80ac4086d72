// kq_lane.hpp -- cross-lane exchange lane <-> lane ^ M of a wave64 without the LDS crossbar: DPP for M < 16
// (quad permutes, row shifts with bank masks, row rotate), v_permlane16_swap / v_permlane32_swap (gfx950) above.
// A ds_bpermute costs an LDS round trip; in the single-wave demodulators forty of them in a dependent chain were
// the whole block latency.
// Also the two helpers that kq_pruned.hip shares with the rest but cannot take from kq_ldsfft.hpp, whose cmul would
// collide with its packed one: the wave-level LDS fence and the unit phasor.  And the PCM word that kq_kernels.hip's
// delivery and kq_mon.hip's buses share.
#pragma once
#include <hip/hip_runtime.h>

namespace kq {

template <int CTRL, int BANK_MASK = 0xF>
__device__ __forceinline__ int dpp_mov(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, BANK_MASK, false);
}

// value of lane (lane ^ M); `lane` is the caller's lane id (only read for M >= 16)
template <int M>
__device__ __forceinline__ int lane_xor_i(int v, int lane) {
  static_assert(M == 1 || M == 2 || M == 4 || M == 8 || M == 16 || M == 32, "power of two below 64");
  if constexpr (M == 1) {
    return dpp_mov<0xB1>(v, v);  // quad_perm [1,0,3,2]
  } else if constexpr (M == 2) {
    return dpp_mov<0x4E>(v, v);  // quad_perm [2,3,0,1]
  } else if constexpr (M == 4) {
    int r = dpp_mov<0x104, 0x5>(v, v);  // row_shl:4 into banks 0 and 2 (lanes with bit 2 clear take lane + 4)
    return dpp_mov<0x114, 0xA>(r, v);   // row_shr:4 into banks 1 and 3
  } else if constexpr (M == 8) {
    return dpp_mov<0x128>(v, v);  // row_ror:8
  } else if constexpr (M == 16) {
    auto const r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    // r[0] = [row0, row0, row2, row2], r[1] = [row1, row1, row3, row3] of v
    return (lane & 16) ? (int)r[0] : (int)r[1];
  } else {
    auto const r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    // r[0] = [low half, low half], r[1] = [high half, high half]
    return (lane & 32) ? (int)r[0] : (int)r[1];
  }
}

template <int M>
__device__ __forceinline__ float lane_xor(float v, int lane) {
  return __int_as_float(lane_xor_i<M>(__float_as_int(v), lane));
}
// both halves of a float2 from lane ^ (1 << s), s a constant after unrolling
__device__ __forceinline__ float2 lane_xor_pow2(float2 v, int s, int lane) {
  switch (s) {
    case 0: return make_float2(lane_xor<1>(v.x, lane), lane_xor<1>(v.y, lane));
    case 1: return make_float2(lane_xor<2>(v.x, lane), lane_xor<2>(v.y, lane));
    case 2: return make_float2(lane_xor<4>(v.x, lane), lane_xor<4>(v.y, lane));
    case 3: return make_float2(lane_xor<8>(v.x, lane), lane_xor<8>(v.y, lane));
    case 4: return make_float2(lane_xor<16>(v.x, lane), lane_xor<16>(v.y, lane));
    default: return make_float2(lane_xor<32>(v.x, lane), lane_xor<32>(v.y, lane));
  }
}

// LDS written by one lane of this wave, read by another
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Unit phasor exp(j*2*pi*turns) from a double phase in turns
__device__ __forceinline__ float2 phasor_turns(double turns) {
  turns -= rint(turns);
  float s, c;
  sincospif(2.0f * (float)turns, &s, &c);
  return make_float2(c, s);
}

// float -> clipped int16 in network byte order, in the low half of the word: scaleclip (audio.c:22-28) and htons
// (audio.c:48,98).  A NaN gives 0
__device__ __forceinline__ unsigned pcm_word_be(float x) {
  int v;
  if (x >= 1.0f)
    v = 32767;
  else if (x <= -1.0f)
    v = -32768;
  else
    v = (int)(32767.f * x);  // truncation, as the (short) cast of audio.c:27
  unsigned const h = (unsigned)v & 0xffffu;
  return ((h << 8) | (h >> 8)) & 0xffffu;
}

}  // namespace kq
