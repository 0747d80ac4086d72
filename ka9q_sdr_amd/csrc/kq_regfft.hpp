// kq_regfft.hpp -- small FFTs held entirely in a thread's registers (compile-time twiddles, fully unrolled), the
// building block of the register-resident transforms (kq_pruned.hip, kq_full16k.hip).  Forward sign (-1),
// unnormalised, like fftwf_plan_dft_1d(FFTW_FORWARD) in filter.c:84.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

namespace kq {
namespace rfft {

// ---- compile-time twiddles exp(-2 pi i k / n), 0 <= k < n/2
constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr double cx_cos(double x) {  // |x| <= pi/4
  double const x2 = x * x;
  double term = 1, sum = 1;
  for (int n = 1; n < 14; n++) {
    term *= -x2 / ((2 * n - 1) * (2 * n));
    sum += term;
  }
  return sum;
}
constexpr double cx_sin(double x) {
  double const x2 = x * x;
  double term = x, sum = x;
  for (int n = 1; n < 14; n++) {
    term *= -x2 / ((2 * n) * (2 * n + 1));
    sum += term;
  }
  return sum;
}
constexpr double turn_cos(double t) {  // cos(2 pi t), 0 <= t < 0.5, octant symmetries keep exact zeros exact
  return t <= 0.125 ? cx_cos(2 * kPi * t) : t <= 0.375 ? -cx_sin(2 * kPi * (t - 0.25)) : -cx_cos(2 * kPi * (0.5 - t));
}
constexpr double turn_sin(double t) {
  return t <= 0.125 ? cx_sin(2 * kPi * t) : t <= 0.375 ? cx_cos(2 * kPi * (t - 0.25)) : cx_sin(2 * kPi * (0.5 - t));
}
constexpr float tw_re(int k, int n) { return (float)turn_cos((double)k / n); }
constexpr float tw_im(int k, int n) { return (float)(-turn_sin((double)k / n)); }

constexpr int bitrev5(int i) {
  return ((i & 1) << 4) | ((i & 2) << 2) | (i & 4) | ((i & 8) >> 2) | ((i & 16) >> 4);
}
constexpr int bitrev4(int i) { return ((i & 1) << 3) | ((i & 2) << 1) | ((i & 4) >> 1) | ((i & 8) >> 3); }

// One radix-2 butterfly of stage LEN: pair index I selects group base = (I / half) * LEN and offset j = I % half.
// FMA-fused: u = a + w b costs 4 fma, the other output is 2a - u (2 fma).
template <int NP, int LEN, int I>
__device__ __forceinline__ void bfly(float2 (&v)[NP]) {
  constexpr int half = LEN / 2, base = (I / half) * LEN, j = I % half;
  constexpr int t = j * (64 / LEN);  // twiddle exp(-2 pi i t / 64), 0..31
  float2 const a = v[base + j], b = v[base + j + half];
  if constexpr (t == 0) {
    v[base + j] = make_float2(a.x + b.x, a.y + b.y);
    v[base + j + half] = make_float2(a.x - b.x, a.y - b.y);
  } else if constexpr (t == 16) {  // w = -i
    v[base + j] = make_float2(a.x + b.y, a.y - b.x);
    v[base + j + half] = make_float2(a.x - b.y, a.y + b.x);
  } else {
    constexpr float wr = tw_re(t, 64), wi = tw_im(t, 64);
    float2 u;
    u.x = fmaf(wr, b.x, fmaf(-wi, b.y, a.x));
    u.y = fmaf(wr, b.y, fmaf(wi, b.x, a.y));
    v[base + j] = u;
    v[base + j + half] = make_float2(fmaf(2.f, a.x, -u.x), fmaf(2.f, a.y, -u.y));
  }
}

template <int NP, int LEN, int... I>
__device__ __forceinline__ void stage(float2 (&v)[NP], std::integer_sequence<int, I...>) {
  if constexpr (LEN <= NP) (bfly<NP, LEN, I>(v), ...);
}

// NP-point forward FFT in registers (NP <= 32), decimation in time, radix 2, unrolled by construction.
// In: sample a stored at v[bitrev(a)].  Out: bin q in v[q].
template <int NP>
__device__ __forceinline__ void fft_dit(float2 (&v)[NP]) {
  using pairs = std::make_integer_sequence<int, NP / 2>;
  stage<NP, 2>(v, pairs{});
  stage<NP, 4>(v, pairs{});
  stage<NP, 8>(v, pairs{});
  stage<NP, 16>(v, pairs{});
  stage<NP, 32>(v, pairs{});
}

// ---- packed variant: a complex value is one 2-vector, so that a butterfly is three v_pk_fma_f32 (two for the
// trivial twiddles) instead of six scalar FMAs.
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
// a * b, complex, for compile-time or scalar-register operands (the compiler picks the encodings)
__device__ __forceinline__ v2f pk_cmul_any(v2f a, v2f b) { return pk_fma((v2f){-a.y, a.y}, b.yx, a.xx * b); }
// a * b, complex, both in vector registers: exactly two instructions.  The half selects and the sign of a.y ride on
// the VOP3P operand modifiers (op_sel / op_sel_hi / neg_lo); written out because the compiler, given the vector form
// above, materialises {-a.y, a.y} with a v_xor_b32 and a v_mov_b32 whenever `a` has a second use.
//   t = (a.x b.x, a.x b.y);  d = (-a.y b.y + t.x, a.y b.x + t.y)
__device__ __forceinline__ v2f pk_cmul(v2f a, v2f b) {
  v2f t, d;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(d) : "v"(a), "v"(b), "v"(t));
  return d;
}
// a * conj(b)
__device__ __forceinline__ v2f pk_cmul_conj(v2f a, v2f b) {
  v2f t, d;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));  // (a.x b.x, -a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b), "v"(t));  // (+a.y b.y, +a.y b.x)
  return d;
}

// c + a * b, complex, all in vector registers: two instructions (the product's first half accumulates onto c)
__device__ __forceinline__ v2f pk_cmadd(v2f a, v2f b, v2f c) {
  v2f t, d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(a), "v"(b), "v"(c));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(d) : "v"(a), "v"(b), "v"(t));
  return d;
}

// a * b with b in scalar registers: pk_cmul's two instructions with one scalar source each.  (pk_cmul_any leaves the
// encodings to the compiler, which then builds {-a.y, a.y} in registers: a v_xor_b32 and a v_mov_b32 per product.)
__device__ __forceinline__ v2f pk_cmul_s(v2f a, v2f b) {
  v2f t, d;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "s"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(d) : "v"(a), "s"(b), "v"(t));
  return d;
}

// ---- block forms: K independent products in ONE asm statement, all first halves, then all second halves.
// The compiler knows no latency for an asm statement and schedules around none: a run of single products comes out as
// mul, fma, mul, fma ..., every instruction waiting for the one before it, with an s_nop 0 between the two statements of
// a product (its hazard recogniser's answer to a register written by one statement and read by the next).  Inside one
// statement a half's neighbours are the other products' halves and nothing is inserted.  Each product is pk_cmul's (or
// pk_cmadd's) two instructions on the same operands with the same modifiers -- the same bits; the first half lands in
// the destination itself, which is early-clobber (the other products' operands are still to be read), so a block holds
// no registers beyond its results.
#define KQ_CM_LO "op_sel_hi:[0,1]"
#define KQ_CM_HI "op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
#define KQ_CMA_LO "op_sel_hi:[0,1,1]"
#define KQ_DEFINE_CMUL_BLOCKS(NAME, BC)                                                                                      \
  __device__ __forceinline__ void NAME##2(v2f &d0, v2f &d1, v2f a0, v2f b0, v2f a1, v2f b1) {                                \
    v2f x0, x1;                                                                                                              \
    asm("v_pk_mul_f32 %0, %2, %4 " KQ_CM_LO "\n\t"                                                                           \
        "v_pk_mul_f32 %1, %3, %5 " KQ_CM_LO "\n\t"                                                                           \
        "v_pk_fma_f32 %0, %2, %4, %0 " KQ_CM_HI "\n\t"                                                                       \
        "v_pk_fma_f32 %1, %3, %5, %1 " KQ_CM_HI                                                                              \
        : "=&v"(x0), "=&v"(x1)                                                                                               \
        : "v"(a0), "v"(a1), BC(b0), BC(b1));                                                                                 \
    d0 = x0, d1 = x1;                                                                                                        \
  }                                                                                                                          \
  __device__ __forceinline__ void NAME##4(v2f &d0, v2f &d1, v2f &d2, v2f &d3, v2f a0, v2f b0, v2f a1, v2f b1, v2f a2,       \
                                          v2f b2, v2f a3, v2f b3) {                                                          \
    v2f x0, x1, x2, x3;                                                                                                      \
    asm("v_pk_mul_f32 %0, %4, %8 " KQ_CM_LO "\n\t"                                                                           \
        "v_pk_mul_f32 %1, %5, %9 " KQ_CM_LO "\n\t"                                                                           \
        "v_pk_mul_f32 %2, %6, %10 " KQ_CM_LO "\n\t"                                                                          \
        "v_pk_mul_f32 %3, %7, %11 " KQ_CM_LO "\n\t"                                                                          \
        "v_pk_fma_f32 %0, %4, %8, %0 " KQ_CM_HI "\n\t"                                                                       \
        "v_pk_fma_f32 %1, %5, %9, %1 " KQ_CM_HI "\n\t"                                                                       \
        "v_pk_fma_f32 %2, %6, %10, %2 " KQ_CM_HI "\n\t"                                                                      \
        "v_pk_fma_f32 %3, %7, %11, %3 " KQ_CM_HI                                                                             \
        : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3)                                                                         \
        : "v"(a0), "v"(a1), "v"(a2), "v"(a3), BC(b0), BC(b1), BC(b2), BC(b3));                                               \
    d0 = x0, d1 = x1, d2 = x2, d3 = x3;                                                                                      \
  }
#define KQ_BC_V(x) "v"(x)
#define KQ_BC_S(x) "s"(x)
KQ_DEFINE_CMUL_BLOCKS(pk_cmul, KQ_BC_V)    // pk_cmul2, pk_cmul4:     d_i = a_i * b_i
KQ_DEFINE_CMUL_BLOCKS(pk_cmul_s, KQ_BC_S)  // pk_cmul_s2, pk_cmul_s4: the same with the b_i in scalar registers
#undef KQ_DEFINE_CMUL_BLOCKS
#undef KQ_BC_V
#undef KQ_BC_S
// d_i = c_i + a_i * b_i (pk_cmadd); c_i may be the variable d_i refers to
__device__ __forceinline__ void pk_cmadd2(v2f &d0, v2f &d1, v2f a0, v2f b0, v2f c0, v2f a1, v2f b1, v2f c1) {
  v2f x0, x1;
  asm("v_pk_fma_f32 %0, %2, %4, %6 " KQ_CMA_LO "\n\t"
      "v_pk_fma_f32 %1, %3, %5, %7 " KQ_CMA_LO "\n\t"
      "v_pk_fma_f32 %0, %2, %4, %0 " KQ_CM_HI "\n\t"
      "v_pk_fma_f32 %1, %3, %5, %1 " KQ_CM_HI
      : "=&v"(x0), "=&v"(x1)
      : "v"(a0), "v"(a1), "v"(b0), "v"(b1), "v"(c0), "v"(c1));
  d0 = x0, d1 = x1;
}
// (No pk_cmadd4: the only run of accumulating products, the unswept N = 65536 mix, is a chain of four per row with two
// rows in hand.)
#undef KQ_CM_LO
#undef KQ_CM_HI
#undef KQ_CMA_LO

template <int NP, int LEN, int I>
__device__ __forceinline__ void bfly_pk(v2f (&v)[NP]) {
  constexpr int half = LEN / 2, base = (I / half) * LEN, j = I % half;
  constexpr int t = j * (64 / LEN);
  v2f const a = v[base + j], b = v[base + j + half];
  if constexpr (t == 0) {
    v[base + j] = a + b;
    v[base + j + half] = a - b;
  } else if constexpr (t == 16) {  // w = -i: a +- (b.y, -b.x).  The swap and the sign ride on the operand modifiers; given the
    // vector expression the compiler builds (b.y, -b.x) in registers first (a v_xor_b32 and a v_mov_b32 per butterfly)
    // (The two as ONE statement -- they are independent of each other -- measured no faster: DESIGN_DIARY.md I, A.1.)
    v2f x, y;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(x) : "v"(a), "v"(b));
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(y) : "v"(a), "v"(b));
    v[base + j] = x;
    v[base + j + half] = y;
  } else {
    constexpr float wr = tw_re(t, 64), wi = tw_im(t, 64);
    v2f const u = pk_fma((v2f){-wi, wi}, b.yx, pk_fma((v2f){wr, wr}, b, a));
    v[base + j] = u;
    v[base + j + half] = pk_fma((v2f){2.f, 2.f}, a, -u);
  }
}

template <int NP, int LEN, int... I>
__device__ __forceinline__ void stage_pk(v2f (&v)[NP], std::integer_sequence<int, I...>) {
  if constexpr (LEN <= NP) (bfly_pk<NP, LEN, I>(v), ...);
}

template <int NP>
__device__ __forceinline__ void fft_dit_pk(v2f (&v)[NP]) {
  using pairs = std::make_integer_sequence<int, NP / 2>;
  stage_pk<NP, 2>(v, pairs{});
  stage_pk<NP, 4>(v, pairs{});
  stage_pk<NP, 8>(v, pairs{});
  stage_pk<NP, 16>(v, pairs{});
  stage_pk<NP, 32>(v, pairs{});
}

}  // namespace rfft
}  // namespace kq
