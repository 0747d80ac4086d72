// kq_fe.hpp -- what kq_fe.hip (raw A/D conditioning) and kq_decim.hip (the cascade, whose first group can read the raw
// samples itself) share: the per-block constant table, the per-sample conditioning in the reference's operand order, and
// the entry point by which a kq_frontend drives a kq_decimator on raw input.  Device functions, so .hip units only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct kq_decimator;

namespace kq {

// One row of the constant table: what hackrf.c:158-174 / funcube.c:331-346 apply to every sample of one block.
constexpr int kFeRow = 8;  // floats per row (32 bytes): DC_i, DC_q, gain_i, gain_q, secphi, tanphi, 0, 0
struct FeConst {
  float dc_i, dc_q, gain_i, gain_q, secphi, tanphi;
};

// Raw input of a call as the kernels see it.  raw[0] is sample `off0` of the block that table row 0 belongs to.
struct FeRaw {
  const void *raw;     // int8 or int16 I,Q pairs, device memory, 16-byte aligned
  const float *table;  // rows for the blocks this call touches
  unsigned block;      // samples per block
  unsigned off0;
  int s16;             // 0: int8, 1: int16
};

__device__ __forceinline__ FeConst fe_row(const float *table, unsigned row) {
  const float4 *p = reinterpret_cast<const float4 *>(table + (size_t)row * kFeRow);
  float4 const a = p[0], b = p[1];
  return FeConst{a.x, a.y, a.z, a.w, b.x, b.y};
}

template <bool S16>
__device__ __forceinline__ float fe_scale() {
  // hackrf.c:78 SCALE8, funcube.c:64 SCALE16: a double quotient stored in a float
  return S16 ? (float)(1. / 32767.) : (float)(1. / 127.);
}

// samples per 16-byte load
template <bool S16>
constexpr int fe_vec() {
  return S16 ? 4 : 8;
}

// hackrf.c:154-174 on one sample whose -128 has already become -127: unfused, in the reference's operand order
template <bool S16>
__device__ __forceinline__ float2 fe_condition(int i, int q, const FeConst &c) {
#pragma clang fp contract(off)
  float x = (float)i * fe_scale<S16>();
  float y = (float)q * fe_scale<S16>();
  x = x - c.dc_i;
  y = y - c.dc_q;
  x = x * c.gain_i;
  y = y * c.gain_q;
  float const a = c.secphi * y;
  float const b = c.tanphi * x;
  y = a - b;
  return make_float2(x, y);
}

// the integer I and Q of sample j of a 16-byte vector of raw samples, with the int8 rule applied (hackrf.c:146-153)
template <bool S16>
__device__ __forceinline__ void fe_unpack(uint4 v, int j, int &i, int &q) {
  unsigned const w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (S16) {
    i = (int)(short)(w[j] & 0xffff);
    q = (int)(short)(w[j] >> 16);
  } else {
    unsigned const h = w[j >> 1] >> ((j & 1) * 16);
    i = max((int)(signed char)(h & 0xff), -127);
    q = max((int)(signed char)((h >> 8) & 0xff), -127);
  }
}

// one sample read on its own (edges): index in samples from `raw`
template <bool S16>
__device__ __forceinline__ void fe_load1(const void *raw, unsigned idx, int &i, int &q) {
  if constexpr (S16) {
    short2 const s = reinterpret_cast<const short2 *>(raw)[idx];
    i = s.x;
    q = s.y;
  } else {
    char2 const s = reinterpret_cast<const char2 *>(raw)[idx];
    i = max((int)(signed char)s.x, -127);
    q = max((int)(signed char)s.y, -127);
  }
}

// Where a sample sits: its table row and its offset inside that row's block.  Positions (off0 + index in the call) fit
// 32 bits: kq_fe_create bounds max_samples.
struct FeSpan {
  unsigned row, rem;
};
__device__ __forceinline__ FeSpan fe_locate(const FeRaw &r, unsigned idx) {
  unsigned const pos = idx + r.off0;
  unsigned const row = pos / r.block;
  return FeSpan{row, pos - row * r.block};
}
// `b` moved on by x samples, b.rem + x < 2^23 (exact in a float): the quotient by a reciprocal, then put right by one
__device__ __forceinline__ FeSpan fe_advance(FeSpan b, unsigned x, unsigned block, float rcp) {
  unsigned const y = b.rem + x;
  unsigned q = (unsigned)((float)y * rcp);
  int rem = (int)(y - q * block);
  if (rem < 0) {
    q--;
    rem += (int)block;
  } else if (rem >= (int)block) {
    q++;
    rem -= (int)block;
  }
  return FeSpan{b.row + q, (unsigned)rem};
}

// sample `idx` of the call, conditioned with its own block's constants
template <bool S16>
__device__ __forceinline__ float2 fe_sample(const FeRaw &r, unsigned idx) {
  int i, q;
  fe_load1<S16>(r.raw, idx, i, q);
  return fe_condition<S16>(i, q, fe_row(r.table, fe_locate(r, idx).row));
}

// The kVec samples of one 16-byte vector whose first sample sits at `s`, conditioned and handed on pair by pair:
// emit(j, sample j, sample j + 1) for j = 0, 2, ...  A vector straddles at most one block boundary (block >= 64); only
// a wave that holds such a vector goes through the per-sample choice of row.
template <bool S16, class Emit>
__device__ __forceinline__ void fe_vector(const FeRaw &r, uint4 v, FeSpan s, Emit emit) {
  constexpr int kVec = fe_vec<S16>();
  FeConst const c = fe_row(r.table, s.row);
  unsigned const lim = r.block - s.rem;  // samples from `lim` on belong to the next row
  if (!__any(lim < (unsigned)kVec)) {
#pragma unroll
    for (int j = 0; j < kVec; j += 2) {
      int i0, q0, i1, q1;
      fe_unpack<S16>(v, j, i0, q0);
      fe_unpack<S16>(v, j + 1, i1, q1);
      emit(j, fe_condition<S16>(i0, q0, c), fe_condition<S16>(i1, q1, c));
    }
  } else {
    // rare for the block sizes in use (one wave in block / 512): the rows are fetched again per sample, which keeps
    // this path's registers below the common one's
#pragma unroll
    for (int j = 0; j < kVec; j += 2) {
      int i0, q0, i1, q1;
      fe_unpack<S16>(v, j, i0, q0);
      fe_unpack<S16>(v, j + 1, i1, q1);
      float2 const w0 = fe_condition<S16>(i0, q0, fe_row(r.table, s.row + ((unsigned)j >= lim)));
      float2 const w1 = fe_condition<S16>(i1, q1, fe_row(r.table, s.row + ((unsigned)j + 1 >= lim)));
      emit(j, w0, w1);
    }
  }
}

typedef unsigned fe_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 fe_load_once(const uint4 *p) {
  fe_u4 const w = __builtin_nontemporal_load(reinterpret_cast<const fe_u4 *>(p));
  return make_uint4(w.x, w.y, w.z, w.w);
}

}  // namespace kq

// kq_decim.hip, for kq_fe_process_decim: where the decimator lives and what it can take
struct kq_decim_internal_info {
  int device;
  void *stream;
  int log_decimate;
  size_t max_out;
};
void kq_decim_internal_get_info(kq_decimator *d, kq_decim_internal_info *out);
// kq_decim_process on raw samples, device memory only, asynchronous on the decimator's stream: the first group reads
// `raw` and conditions it in registers; the carried history stays conditioned complex float
int kq_decim_internal_process_raw(kq_decimator *d, const kq::FeRaw &raw, size_t n_out, float *out_cf32, int16_t *out_s16,
                                  float *out_energy);
