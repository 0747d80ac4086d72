// kq_fftplan.cpp -- FFT planning on the host: which sizes the kernels transform (fft_size_ok), the plan of a size on the
// generic path (fft_dim), the half-circle twiddle table of lds_fft / fft_any (half_twiddles), and the one place where a
// table is uploaded once per device and never freed (upload_once).  Host only: no kernel here.  Declared in kq_device.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "kq_device.hpp"

namespace kq {

// Tables outlive the handle that asked first (a later handle on the same device finds them), so nothing ever frees one.
const void *upload_once(int table, int size, size_t bytes, const std::function<void(void *)> &fill) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, void *> tabs;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = tabs.find({dev, table, size});
  if (it != tabs.end()) return it->second;
  std::vector<char> h(bytes);
  fill(h.data());
  void *d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  tabs[{dev, table, size}] = d;
  return d;
}

// half-circle twiddle tables exp(-2 pi i k / T), k < T/2, per device and size (built in double, rounded once)
const float2 *half_twiddles(int log2T) {
  size_t const T = (size_t)1 << log2T;
  return (const float2 *)upload_once(TABLE_HALF_TWIDDLES, log2T, (T / 2 ? T / 2 : 1) * sizeof(float2), [T](void *bytes) {
    float2 *h = (float2 *)bytes;
    for (size_t k = 0; k < T / 2; k++) {
      double const a = -2.0 * M_PI * (double)k / (double)T;
      h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  });
}

bool fft_size_ok(int n) {
  if (n < 2 || n > 65536 || (n & 1)) return false;
  for (int p : {2, 3, 5, 7})
    while (n % p == 0) n /= p;
  return n == 1;
}

// The plan of an n-point transform on the generic path, tables on the current device (cached per device and size)
FftDim fft_dim(int n, bool *ok) {
  FftDim d{};
  d.n = n;
  d.log2n = -1;
  if (ok) *ok = false;
  if (n >= 1 && (n & (n - 1)) == 0) {
    d.log2n = 0;
    while ((1 << d.log2n) < n) d.log2n++;
    if (ok) *ok = true;
    return d;
  }
  {  // (odd sizes are fine here -- a factor of a two-pass transform may be one; fft_size_ok's evenness is the filters' rule)
    int m = n;
    for (int p : {2, 3, 5, 7})
      while (m % p == 0) m /= p;
    if (n < 2 || n > 65536 || m != 1) return d;
  }
  {  // radices: 4s first (fewest passes), then 2, 3s, 5s, 7s
    int m = n;
    while (m % 4 == 0) d.f[d.nf++] = 4, m /= 4;
    while (m % 2 == 0) d.f[d.nf++] = 2, m /= 2;
    while (m % 3 == 0) d.f[d.nf++] = 3, m /= 3;
    while (m % 5 == 0) d.f[d.nf++] = 5, m /= 5;
    while (m % 7 == 0) d.f[d.nf++] = 7, m /= 7;
  }
  d.rev = (const unsigned short *)upload_once(TABLE_DIM_REV, n, n * sizeof(unsigned short), [n, &d](void *bytes) {
    unsigned short *rev = (unsigned short *)bytes;
    for (int p = 0; p < n; p++) {  // position p = sum_k d_k prod_{j<k} f_j holds index i = sum_k d_k n / prod_{j<=k} f_j
      int rest = p, weight = n, i = 0;
      for (int k = 0; k < d.nf; k++) {
        weight /= d.f[k];
        i += (rest % d.f[k]) * weight;
        rest /= d.f[k];
      }
      rev[i] = (unsigned short)p;
    }
  });
  d.twc = (const float2 *)upload_once(TABLE_DIM_TW, n, n * sizeof(float2), [n](void *bytes) {
    float2 *tw = (float2 *)bytes;
    for (int k = 0; k < n; k++) {
      double const a = -2.0 * M_PI * (double)k / (double)n;
      tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  });
  if (!d.rev || !d.twc) {
    d.rev = nullptr;
    d.twc = nullptr;
    return d;
  }
  d.tw_n = n;
  if (ok) *ok = true;
  return d;
}

}  // namespace kq
