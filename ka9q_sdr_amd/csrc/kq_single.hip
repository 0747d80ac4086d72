// kq_single.hip -- one transform at a time on data resident on the device: the kernels behind the compat surface
// (kq_compat.cpp), the demodulator entry points (kq_radio.cpp) and kq_bank_process_spectrum.
//
//   k_fft_single                 one transform of up to 16384 points in LDS
//   k_fft_cols / k_fft_rows      larger ones, N = Na * Nb through global memory (launch_fft_large)
//   k_n0_single                  compute_n0 (radio.c:383-425) on a master spectrum
//   k_slave_single               one slave execution, all four in/out type combinations of filter.c:206-250
//   k_slave_bank                 the bank's slave on a spectrum handed in from outside
#include "kq_device.hpp"
#include "kq_ldsfft.hpp"

namespace kq {

// ---------------------------------------------------------------- single transforms (compat surface)
__global__ void k_fft_single(const float2 *__restrict__ in, float2 *__restrict__ out, FftDim d, int sign,
                             const float2 *__restrict__ tw, int tw_log2) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int const n = d.n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) lds[fft_pos((unsigned)i, d)] = in[i];
  if (sign < 0)
    fft_any<-1>(lds, d, tw, tw_log2);
  else
    fft_any<+1>(lds, d, tw, tw_log2);
  for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = lds[i];
}

// n: a power of two (tw / tw_log2: the half-circle table lds_fft reads) or any 2^a 3^b 5^c 7^d the caller has a plan for
void launch_fft_single(hipStream_t s, const float2 *in, float2 *out, const FftDim &d, int sign, const float2 *tw, int tw_log2) {
  size_t const lds_bytes = sizeof(float2) * (size_t)d.n;
  ensure_dynamic_lds((const void *)k_fft_single, lds_bytes);
  int const threads = d.n >= 4096 ? 1024 : 256;
  hipLaunchKernelGGL(k_fft_single, dim3(1), dim3(threads), lds_bytes, s, in, out, d, sign, tw, tw_log2);
}

// Transforms beyond the 16384 points one workgroup holds in LDS (compat masters up to 2^22 points): N = Na * Nb through
// global memory.  With n = Nb n1 + n2 and k = k1 + Na k2:
//   X[k1 + Na k2] = sum_n2 W_Nb^{n2 k2} W_N^{n2 k1} sum_n1 x[Nb n1 + n2] W_Na^{n1 k1}
// k_fft_cols: one workgroup per n2 runs the Na-point transform over n1, applies W_N^{n2 k1}, stores tmp[k1][n2];
// k_fft_rows: one workgroup per k1 runs the Nb-point transform over n2 and scatters to out[k1 + Na k2].
// (powers of two: da / db carry log2 and the W_N^{n2 k1} factors come from the half-circle table; otherwise twN is the
// full-circle table of N points and n2 k1 < N indexes it directly)
__global__ void k_fft_cols(const float2 *__restrict__ in, float2 *__restrict__ tmp, FftDim da, FftDim db, int sign,
                           const float2 *__restrict__ tw, int tw_log2, const float2 *__restrict__ twN) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int const na = da.n, nb = db.n, n2 = blockIdx.x;
  for (int i = threadIdx.x; i < na; i += blockDim.x) lds[fft_pos((unsigned)i, da)] = in[(size_t)nb * i + n2];
  if (sign < 0)
    fft_any<-1>(lds, da, tw, tw_log2);
  else
    fft_any<+1>(lds, da, tw, tw_log2);
  if (twN) {
    for (int k1 = threadIdx.x; k1 < na; k1 += blockDim.x) {
      float2 w = twN[(size_t)n2 * k1];
      if (sign > 0) w.y = -w.y;
      tmp[(size_t)k1 * nb + n2] = cmul(lds[k1], w);
    }
    return;
  }
  unsigned const half = 1u << (tw_log2 - 1), shift = (unsigned)(tw_log2 - da.log2n - db.log2n);
  for (int k1 = threadIdx.x; k1 < na; k1 += blockDim.x) {
    unsigned e = ((unsigned)n2 * (unsigned)k1) << shift;  // exponent on the table's period, < 2^tw_log2
    float2 w = tw[e & (half - 1)];
    if (e & half) w = make_float2(-w.x, -w.y);
    if (sign > 0) w.y = -w.y;
    tmp[(size_t)k1 * nb + n2] = cmul(lds[k1], w);
  }
}
__global__ void k_fft_rows(const float2 *__restrict__ tmp, float2 *__restrict__ out, FftDim da, FftDim db, int sign,
                           const float2 *__restrict__ tw, int tw_log2) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int const na = da.n, nb = db.n, k1 = blockIdx.x;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) lds[fft_pos((unsigned)i, db)] = tmp[(size_t)k1 * nb + i];
  if (sign < 0)
    fft_any<-1>(lds, db, tw, tw_log2);
  else
    fft_any<+1>(lds, db, tw, tw_log2);
  for (int k2 = threadIdx.x; k2 < nb; k2 += blockDim.x) out[(size_t)k1 + (size_t)na * k2] = lds[k2];
}

// N beyond one LDS block: a power of two up to 2^22, or 2^a 3^b 5^c 7^d up to 65536 (the full-circle table's reach)
int launch_fft_large(hipStream_t s, const float2 *in, float2 *out, float2 *tmp, int N, int sign, const float2 *tw, int tw_log2) {
  bool ok = false;
  FftDim const dn = fft_dim(N, &ok);
  if (!ok) return -1;
  int na, nb;
  if (dn.log2n >= 0) {
    int const log2na = (dn.log2n + 1) / 2;
    na = 1 << log2na;
    nb = N >> log2na;
  } else {  // split the radices so that both sides fit one LDS block and stay even where they can
    na = 1;
    for (int k = 0; k < dn.nf; k++)
      if ((long long)na * na < N) na *= dn.f[k];
    nb = N / na;
    if (na > 16384 || nb > 16384) return -1;
  }
  bool oka = false, okb = false;
  FftDim const da = fft_dim(na, &oka), db = fft_dim(nb, &okb);
  if (!oka || !okb) return -1;
  size_t const lds_a = sizeof(float2) * (size_t)na, lds_b = sizeof(float2) * (size_t)nb;
  ensure_dynamic_lds((const void *)k_fft_cols, lds_a);
  ensure_dynamic_lds((const void *)k_fft_rows, lds_b);
  int const ta = na >= 1024 ? 256 : 64, tb = nb >= 1024 ? 256 : 64;
  hipLaunchKernelGGL(k_fft_cols, dim3((unsigned)nb), dim3(ta), lds_a, s, in, tmp, da, db, sign, tw, tw_log2,
                     dn.log2n >= 0 ? (const float2 *)nullptr : dn.twc);
  hipLaunchKernelGGL(k_fft_rows, dim3((unsigned)na), dim3(tb), lds_b, s, tmp, out, da, db, sign, tw, tw_log2);
  return 0;
}

// compute_n0 (radio.c:383-425) on one resident master spectrum (the compat surface and the demodulator entry points)
__global__ void k_n0_single(const float2 *__restrict__ X, int N, int samprate, float low, float high, float *__restrict__ out) {
  __shared__ float red_f[16];
  __shared__ int red_i[16];
  float avg = INFINITY;
  for (int iter = 0; iter < 2; iter++) {
    float acc = 0;
    int bins = 0;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      int const k = (n <= N / 2) ? n : n - N;
      int const prod = (int)((unsigned)k * (unsigned)samprate);  // the reference's 32-bit product, wrap included
      float const f = (float)prod / N;
      if (f >= low && f <= high) continue;
      float const p = cnrm(X[n]);
      if (p < avg * 2) {
        acc += p;
        bins++;
      }
    }
    block_sum_fi(acc, bins, red_f, red_i);
    avg = acc / bins;
  }
  if (threadIdx.x == 0) *out = (float)(avg / (2.0 * N * samprate));
}

void launch_n0_single(hipStream_t s, const float2 *fdomain, int N, int samprate, float low, float high, float *out) {
  hipLaunchKernelGGL(k_n0_single, dim3(1), dim3(1024), 0, s, fdomain, N, samprate, low, high, out);
}

// One slave execution on a resident master spectrum: all four in/out type combinations of
// filter.c:206-250.  out: N_dec float2 (complex out) or N_dec floats packed in float2[N_dec/2] (real out).
__global__ void k_slave_single(const float2 *__restrict__ X, const float2 *__restrict__ H, float2 *__restrict__ out, int N,
                               FftDim dd, int in_real, int out_type, const float2 *__restrict__ tw, int tw_log2) {
  extern __shared__ __attribute__((aligned(16))) float2 G[];
  int const Ndec = dd.n;
  bool const out_real = out_type == 3;
  for (int p = threadIdx.x; p <= Ndec / 2; p += blockDim.x) {
    float2 gp = cmul(H[p], X[p]);
    bool const interior = p > 0 && p < Ndec / 2;
    int const k = Ndec - p;
    float2 gn = make_float2(0, 0);
    if (interior) {
      if (in_real) {
        if (!out_real) gn = cmul(H[k], cconj(X[p]));  // filter.c:214-216
      } else if (!out_real) {
        gn = cmul(H[k], X[N - p]);  // filter.c:225-227
      } else {
        gp = cadd(gp, cconj(cmul(H[k], X[N - p])));  // filter.c:232-234
      }
      if (out_type == 2) {  // CROSS_CONJ, filter.c:239-249
        float2 const pos = gp, neg = gn;
        gp = cadd(pos, cconj(neg));
        gn = csub(neg, cconj(pos));
      }
      if (out_real) gn = cconj(gp);  // c2r Hermitian extension
      G[fft_pos((unsigned)k, dd)] = gn;
    } else if (out_real) {
      gp.y = 0;  // c2r ignores the imaginary parts of DC and Nyquist
    }
    G[fft_pos((unsigned)p, dd)] = gp;
  }
  fft_any<+1>(G, dd, tw, tw_log2);
  if (out_real) {
    float *o = reinterpret_cast<float *>(out);
    for (int i = threadIdx.x; i < Ndec; i += blockDim.x) o[i] = G[i].x;
  } else {
    for (int i = threadIdx.x; i < Ndec; i += blockDim.x) out[i] = G[i];
  }
}

// The bank's slave on a spectrum handed in from outside (kq_bank_process_spectrum): COMPLEX in, COMPLEX or CROSS_CONJ out,
// the last `olen` of the N_dec outputs (filter.c:131) to `out`.
__global__ void k_slave_bank(const float2 *__restrict__ X, const float2 *__restrict__ H, float2 *__restrict__ out, int N, FftDim dd,
                             int olen, int out_type, const float2 *__restrict__ tw, int tw_log2) {
  extern __shared__ __attribute__((aligned(16))) float2 G[];
  int const Ndec = dd.n;
  for (int p = threadIdx.x; p <= Ndec / 2; p += blockDim.x) {
    float2 gp = cmul(H[p], X[p]);
    if (p > 0 && p < Ndec / 2) {
      int const k = Ndec - p;
      float2 gn = cmul(H[k], X[N - p]);  // filter.c:225-227
      if (out_type == 2) {               // CROSS_CONJ, filter.c:239-249
        float2 const pos = gp, neg = gn;
        gp = cadd(pos, cconj(neg));
        gn = csub(neg, cconj(pos));
      }
      G[fft_pos((unsigned)k, dd)] = gn;
    }
    G[fft_pos((unsigned)p, dd)] = gp;
  }
  fft_any<+1>(G, dd, tw, tw_log2);
  for (int i = threadIdx.x; i < olen; i += blockDim.x) out[i] = G[Ndec - olen + i];
}

void launch_slave_bank(hipStream_t s, const float2 *fdomain, const float2 *resp, float2 *out, int N, int Ndec, int olen,
                       int out_type, const float2 *tw, int tw_log2) {
  bool ok = false;
  FftDim const dd = fft_dim(Ndec, &ok);  // (cached: the bank / the compat slave made the plan when it was created)
  if (!ok) return;
  size_t const lds_bytes = sizeof(float2) * (size_t)Ndec;
  ensure_dynamic_lds((const void *)k_slave_bank, lds_bytes);
  int const threads = Ndec >= 4096 ? 1024 : 256;
  hipLaunchKernelGGL(k_slave_bank, dim3(1), dim3(threads), lds_bytes, s, fdomain, resp, out, N, dd, olen, out_type, tw, tw_log2);
}

void launch_slave_single(hipStream_t s, const float2 *fdomain, const float2 *resp, float2 *out, int N, int Ndec, int in_real,
                         int out_type, const float2 *tw, int tw_log2) {
  bool ok = false;
  FftDim const dd = fft_dim(Ndec, &ok);
  if (!ok) return;
  size_t const lds_bytes = sizeof(float2) * (size_t)Ndec;
  ensure_dynamic_lds((const void *)k_slave_single, lds_bytes);
  int const threads = Ndec >= 4096 ? 1024 : 256;
  hipLaunchKernelGGL(k_slave_single, dim3(1), dim3(threads), lds_bytes, s, fdomain, resp, out, N, dd, in_real, out_type, tw, tw_log2);
}

}  // namespace kq
