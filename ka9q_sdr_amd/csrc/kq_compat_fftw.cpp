// kq_compat_fftw.cpp -- the FFTW entry points the reference calls OUTSIDE filter.c (include/ka9q_hip_fftw.h): fm.c:226-228,
// 255,281-283 (the PL tone's 16384-point r2c transform), linear.c:90-92,178,313-317 (the carrier search's 65536-point
// transform), the allocators of fm.c:56,208 / modulate.c:115 (responses handed to create_filter_output, which frees them with
// free(): these allocate with aligned_alloc), and main.c:102-103,183-184 (wisdom / threads: nothing to do).  With them
// `fm.o` / `linear.o` / `main.o` link against this library alone -- no libfftw3f on the link line.
// A plan is (size, kind, the caller's two buffers) on the transform the filter masters use (kq_compat.hpp); fftwf_execute
// moves one transform over the link and back.
#include <cstdlib>

#include "../../include/ka9q_hip_compat.h"
#include "kq_compat.hpp"

using namespace kq::compat;

struct kq_fftwf_plan_s : Transform {
  int kind = 0;  // 0: c2c (sign), 1: r2c, 2: c2r
  int sign = -1;
  void *in = nullptr, *out = nullptr;
};

extern "C" void fftwf_destroy_plan(kq_fftwf_plan_s *p);

static kq_fftwf_plan_s *fftw_plan_make(int n, int kind, int sign, void *in, void *out) {
  if (!Transform::size_ok(n, 2, in && out, "fftwf_plan: size ")) return nullptr;
  if (!ctx_init()) return nullptr;
  CompatScope dev_scope_;
  auto *p = new kq_fftwf_plan_s();
  p->kind = kind;
  p->sign = sign;
  p->in = in;
  p->out = out;
  if (p->create(n)) {
    fftwf_destroy_plan(p);
    return nullptr;
  }
  return p;
}

extern "C" {

void *fftwf_malloc(size_t n) { return aligned_alloc(64, (n + 63) & ~(size_t)63); }
float *fftwf_alloc_real(size_t n) { return static_cast<float *>(fftwf_malloc(n * sizeof(float))); }
kq_cfloat *fftwf_alloc_complex(size_t n) { return static_cast<kq_cfloat *>(fftwf_malloc(n * sizeof(kq_cfloat))); }
void fftwf_free(void *p) { free(p); }

kq_fftwf_plan_s *fftwf_plan_dft_1d(int n, kq_cfloat *in, kq_cfloat *out, int sign, unsigned) {
  return fftw_plan_make(n, 0, sign < 0 ? -1 : +1, in, out);
}
kq_fftwf_plan_s *fftwf_plan_dft_r2c_1d(int n, float *in, kq_cfloat *out, unsigned) { return fftw_plan_make(n, 1, -1, in, out); }
kq_fftwf_plan_s *fftwf_plan_dft_c2r_1d(int n, kq_cfloat *in, float *out, unsigned) { return fftw_plan_make(n, 2, +1, in, out); }

void fftwf_execute(const kq_fftwf_plan_s *cp) {
  auto *p = const_cast<kq_fftwf_plan_s *>(cp);
  if (!p) return;
  CompatScope dev_scope_;
  int const n = p->n;
  const void *src = p->in;
  if (p->kind == 1) {  // real samples in
    src = p->expand_real(static_cast<const float *>(p->in));
  } else if (p->kind == 2) {  // n/2 + 1 bins in: Hermitian extension, DC and Nyquist taken as real (FFTW's c2r)
    const float2 *X = static_cast<const float2 *>(p->in);
    p->stage[0] = make_float2(X[0].x, 0.f);
    p->stage[n / 2] = make_float2(X[n / 2].x, 0.f);
    for (int k = 1; k < n / 2; k++) {
      p->stage[k] = X[k];
      p->stage[n - k] = make_float2(X[k].x, -X[k].y);
    }
    src = p->stage.data();
  }
  std::lock_guard<std::mutex> lk(ctx().mu);  // one transform at a time on the context's stream
  if (p->queue(src, p->sign)) return;
  if (p->kind == 2) {
    if (p->fetch(p->stage.data(), n)) return;
    float *y = static_cast<float *>(p->out);
    for (int i = 0; i < n; i++) y[i] = p->stage[i].x;
    return;
  }
  (void)p->fetch(p->out, p->kind == 1 ? (size_t)n / 2 + 1 : (size_t)n);
}

void fftwf_destroy_plan(kq_fftwf_plan_s *p) {
  if (!p) return;
  CompatScope dev_scope_;
  p->close();
  delete p;
}

// main.c:102-103,183-184: FFTW's wisdom and threading have no counterpart here
int fftwf_import_system_wisdom(void) { return 1; }
void fftwf_make_planner_thread_safe(void) {}
int fftwf_init_threads(void) { return 1; }
void fftwf_plan_with_nthreads(int) {}

}  // extern "C"
