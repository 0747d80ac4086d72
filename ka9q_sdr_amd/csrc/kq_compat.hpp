// kq_compat.hpp -- what the units of the compat surface share (kq_compat.cpp: the filter API; kq_compat_fftw.cpp: the FFTW
// names): the process-wide context -- one device, one stream -- and the n-point transform both surfaces are built on.
// Internal; kq_compat_osc.cpp is host arithmetic and needs none of it.
#pragma once
#include <cstdio>
#include <mutex>
#include <vector>

#include "kq_device.hpp"
#include "kq_host.hpp"

namespace kq::compat {

// The compat surface runs on the device that was current at its first use, on one stream of its own; never closed.
struct Ctx : kq::HostSide {
  bool ok = false;
  int device = 0;
  float *d_scalar = nullptr;  // one float of device scratch (kq_compat_compute_n0)
  std::mutex mu;              // the scratch float; one fftwf_execute at a time
};
Ctx &ctx();       // kq_compat.cpp
bool ctx_init();  // false (and a line on stderr) without a device

// every entry point runs on the context's device and leaves the calling thread's as it found it
struct CompatScope : kq::DeviceScope {
  CompatScope() : DeviceScope(ctx().ok ? ctx().device : -1) {}
};

inline int ilog2(unsigned v) {
  int l = 0;
  while ((1u << l) < v) l++;
  return l;
}

// One n-point complex transform on the context's stream: a filter master (struct filter_in::fwd_plan) or an FFTW plan
struct Transform : kq::HostSide {
  int n = 0, log2T = 0;        // log2T: the half-circle table of the next power of two
  kq::FftDim dim{};
  const float2 *tw = nullptr;  // kq::half_twiddles(log2T): shared, not the transform's to free
  float2 *d_in = nullptr, *d_out = nullptr;
  float2 *d_tmp = nullptr;     // n > 16384: scratch of the two-pass transform
  std::vector<float2> stage;   // n host elements: input that is not n complex samples as it comes is expanded here

  // FFTW plans any n (filter.c:78); here: a power of two up to 2^22, or 2^a 3^b 5^c 7^d (even) up to 65536, and no less than
  // `least`.  args_ok: what else the caller asks of its arguments.  `who`: the caller's name and its word for n
  static bool size_ok(long long n, int least, bool args_ok, const char *who) {
    bool const pow2 = n > 0 && (n & (n - 1)) == 0;
    if (args_ok && n >= least && (pow2 ? n <= (1 << 22) : kq::fft_size_ok((int)n))) return true;
    fprintf(stderr, "ka9q_hip: %s%lld must be a power of two %s4194304 or an even 2^a 3^b 5^c 7^d up to 65536\n", who, n,
            least == 4 ? "in 4.." : "up to ");
    return false;
  }

  // wants ctx_init() done and the context's device current; a failed one is close()d by its owner's delete
  int create(int n_) {
    n = n_;
    log2T = ilog2((unsigned)n);
    if (open_stream(ctx().stream)) return -1;
    bool dim_ok = false;
    dim = kq::fft_dim(n, &dim_ok);
    if (!dim_ok || !(tw = kq::half_twiddles(log2T))) return -1;
    stage.resize(n);
    if (alloc(&d_in, n) || alloc(&d_out, n) || (n > 16384 && alloc(&d_tmp, n))) return -1;
    return 0;
  }

  const float2 *expand_real(const float *x) {
    for (int i = 0; i < n; i++) stage[i] = make_float2(x[i], 0.f);
    return stage.data();
  }

  // upload of n samples and the transform, queued on the stream (the caller may hold a lock of its own around it) ...
  int queue(const void *src, int sign) {
    KQ_TRY(hipMemcpyAsync(d_in, src, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, stream));
    if (n > 16384) return kq::launch_fft_large(stream, d_in, d_out, d_tmp, n, sign, tw, log2T) ? -1 : 0;
    kq::launch_fft_single(stream, d_in, d_out, dim, sign, tw, log2T);
    return 0;
  }

  // ... and the first `bins` of the result copied back and waited for
  int fetch(void *dst, size_t bins) {
    KQ_TRY(hipMemcpyAsync(dst, d_out, bins * sizeof(float2), hipMemcpyDeviceToHost, stream));
    KQ_TRY(hipStreamSynchronize(stream));
    return 0;
  }
};

}  // namespace kq::compat
