// kq_window.hpp -- host-side response design of the satellite banks that shape their own filters (kq_wfm, kq_rds): an
// ideal response on the N bins through window_filter's procedure (filter.c:365-413) in double.  Host only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

#include "kq_design.hpp"

namespace kq {

using cd = std::complex<double>;

// unnormalised DFT, exp(sign 2 pi i k n / N), recursive mixed radix (N = 2^a 3^b 5^c 7^d)
inline void dft_rec(const cd *in, size_t stride, cd *out, int n, int sign) {
  if (n == 1) {
    out[0] = in[0];
    return;
  }
  int p = 2;
  while (n % p) p++;
  int const m = n / p;
  for (int r = 0; r < p; r++) dft_rec(in + r * stride, stride * p, out + (size_t)r * m, m, sign);
  std::vector<cd> acc((size_t)n);
  for (int k = 0; k < n; k++) {
    int const kk = k % m;
    cd s = 0.0;
    for (int r = 0; r < p; r++) {
      long const e = ((long)r * k) % n;
      double const ang = sign * 2.0 * M_PI * (double)e / n;
      s += out[(size_t)r * m + kk] * cd(std::cos(ang), std::sin(ang));
    }
    acc[k] = s;
  }
  std::copy(acc.begin(), acc.end(), out);
}
inline std::vector<cd> dft(const std::vector<cd> &x, int sign) {
  std::vector<cd> out(x.size());
  dft_rec(x.data(), 1, out.data(), (int)x.size(), sign);
  return out;
}

// window_filter (filter.c:365-413) in double: R on the N bins -> H; returned as float H / N (the kernels' transforms are
// unnormalised)
inline std::vector<float2> window_design(const std::vector<cd> &R, int M, double beta) {
  int const N = (int)R.size();
  std::vector<cd> t = dft(R, +1);
  std::vector<double> w(M);
  double const den = kq::i0_double(M_PI * beta);
  for (int n = 0; n < M; n++) {
    double const pp = 2.0 * n / (M - 1) - 1.0;
    w[n] = kq::i0_double(M_PI * beta * std::sqrt(std::max(0.0, 1.0 - pp * pp))) / den;
  }
  std::vector<cd> bb((size_t)N, 0.0);
  for (int n = 0; n < M; n++) bb[n] = t[(size_t)((n - M / 2 + N) % N)] * w[n] / (double)N;
  std::vector<cd> H = dft(bb, -1);
  std::vector<float2> out((size_t)N);
  for (int k = 0; k < N; k++) out[k] = make_float2((float)(H[k].real() / N), (float)(H[k].imag() / N));
  return out;
}
inline double bin_hz(int k, int N, double Fc) { return (k < N / 2 ? k : k - N) * Fc / N; }

}  // namespace kq
