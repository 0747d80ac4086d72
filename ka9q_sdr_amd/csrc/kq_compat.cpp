// kq_compat.cpp -- the reference's one-channel filter API on top of the gfx950 kernels (include/ka9q_hip_compat.h).
// Blocking, one block per call, host buffers at the boundary exactly as the reference's callers expect (radio.c:139-142
// fills input.c[]; linear.c:211 reads output.c[]).
//
// This unit owns the context (kq_compat.hpp), the filter API -- create / execute / delete of masters and slaves, set_filter,
// noise_gain --, the snapshots the demodulator threads take of a master (kq_radio.cpp), kq_compat_compute_n0 and the design
// wrappers.  The FFTW names are kq_compat_fftw.cpp's, the oscillator and dsp.h helpers kq_compat_osc.cpp's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ka9q_hip_radio.h"
#include "kq_compat.hpp"
#include "kq_design.hpp"

using namespace kq::compat;

namespace kq::compat {

Ctx &ctx() {
  static Ctx c;
  return c;
}

bool ctx_init() {
  Ctx &c = ctx();
  std::lock_guard<std::mutex> lk(c.mu);
  if (c.ok) return true;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    fprintf(stderr, "ka9q_hip: no HIP device; the filter API has no CPU fallback\n");
    return false;
  }
  if (hipGetDevice(&c.device) != hipSuccess) return false;
  if (!c.stream && c.open_stream(nullptr)) return false;
  if (c.alloc(&c.d_scalar, 1)) return false;
  c.ok = true;
  return true;
}

}  // namespace kq::compat

namespace {

struct MasterDev : Transform {
  // which block's samples d_in holds, as of the work queued so far: the upload and this number move together under
  // in_mu, so a reader that queues its copy under the same lock knows which block it will get (compat_snapshot_window)
  std::mutex in_mu;
  unsigned in_block = 0;
};

struct SlaveDev : kq::HostSide {
  int Ndec = 0;
  float2 *d_resp = nullptr, *d_out = nullptr;
};

inline float re(kq_cfloat z) { return __real__ z; }
inline float im(kq_cfloat z) { return __imag__ z; }

// a device-to-device copy of one of the master's N-element buffers, queued under in_mu (the block it carries is the one
// recorded with the last upload queued) and waited for
int snapshot(MasterDev *d, const float2 *src, float2 *dst, unsigned *block) {
  {
    std::lock_guard<std::mutex> lk(d->in_mu);
    KQ_TRY(hipMemcpyAsync(dst, src, (size_t)d->n * sizeof(float2), hipMemcpyDeviceToDevice, d->stream));
    if (block) *block = d->in_block;
  }
  KQ_TRY(hipStreamSynchronize(d->stream));
  return d->n;
}

}  // namespace

namespace kq {

int compat_master_device(void) { return ctx().ok ? ctx().device : -1; }

// The master may already have queued the next block's upload (it does not wait for its consumers, filter.c:146-172):
// the copy lands in stream order
int compat_snapshot_window(struct filter_in *m, float2 *dst, unsigned *block) {
  if (!m || !m->fwd_plan || !dst) return -1;
  CompatScope dev_scope_;
  MasterDev *d = (MasterDev *)m->fwd_plan;
  return snapshot(d, d->d_in, dst, block);
}

// The master's spectrum of the block last transformed (N bins, complex input): what execute_filter_output and
// compute_n0 read in the reference (filter.c:206-227, radio.c:396), copied so that the master may go on to its next block.
int compat_snapshot_spectrum(struct filter_in *m, float2 *dst, unsigned *block) {
  if (!m || !m->fwd_plan || !dst || m->in_type != COMPLEX) return -1;
  CompatScope dev_scope_;
  MasterDev *d = (MasterDev *)m->fwd_plan;
  return snapshot(d, d->d_out, dst, block);
}

}  // namespace kq

extern "C" {

float Kaiser_beta = 3.0;

float kq_compat_compute_n0(struct filter_in *m, int samprate, float low, float high) {
  if (!m || !m->fwd_plan || m->in_type != COMPLEX || samprate <= 0) return NAN;
  CompatScope dev_scope_;
  MasterDev *d = (MasterDev *)m->fwd_plan;
  Ctx &c = ctx();
  float r = NAN;
  std::lock_guard<std::mutex> lk(c.mu);  // one scratch float
  kq::launch_n0_single(c.stream, d->d_out, d->n, samprate, low, high, c.d_scalar);
  if (hipMemcpyAsync(&r, c.d_scalar, sizeof r, hipMemcpyDeviceToHost, c.stream) != hipSuccess) return NAN;
  if (hipStreamSynchronize(c.stream) != hipSuccess) return NAN;
  return r;
}

struct filter_in *create_filter_input(unsigned int L, unsigned int M, enum filtertype in_type) {
  unsigned const N = L + M - 1;
  if (!Transform::size_ok(N, 4, L != 0 && M != 0, "create_filter_input: N=")) return NULL;
  if (!ctx_init()) return NULL;
  CompatScope dev_scope_;
  struct filter_in *m = (struct filter_in *)calloc(1, sizeof(*m));
  if (!m) return NULL;
  pthread_mutex_init(&m->filter_mutex, NULL);
  pthread_cond_init(&m->filter_cond, NULL);
  if (in_type != REAL && in_type != COMPLEX) {
    fprintf(stderr, "Filter input type %d, assuming complex\n", in_type);  // filter.c:69-71
    in_type = COMPLEX;
  }
  m->in_type = in_type;
  m->ilen = L;
  m->impulse_length = M;
  MasterDev *d = new MasterDev();
  m->fwd_plan = d;
  if (d->create((int)N)) {  // (its half-circle table is also what the slaves are handed)
    delete_filter_input(m);
    return NULL;
  }
  if (in_type == COMPLEX) {
    m->fdomain = (kq_cfloat *)calloc(N, sizeof(kq_cfloat));
    m->input_buffer.c = (kq_cfloat *)calloc(N, sizeof(kq_cfloat));  // history cleared: filter.c:76
    m->input.c = m->input_buffer.c + (M - 1);
  } else {
    m->fdomain = (kq_cfloat *)calloc(N / 2 + 1, sizeof(kq_cfloat));
    m->input_buffer.r = (float *)calloc(N, sizeof(float));
    m->input.r = m->input_buffer.r + (M - 1);
  }
  return m;
}

int execute_filter_input(struct filter_in *m) {
  if (m == NULL) return -1;  // filter.c:148-149
  CompatScope dev_scope_;
  MasterDev *d = (MasterDev *)m->fwd_plan;
  int const N = d->n;
  const void *src = m->in_type == REAL ? (const void *)d->expand_real(m->input_buffer.r) : m->input_buffer.c;
  {
    // upload and transform are queued under one lock: a consumer's snapshot (queued under the same lock) then finds
    // window, spectrum and block number of ONE block, whichever side of this pair it lands on
    std::lock_guard<std::mutex> lk(d->in_mu);
    if (d->queue(src, -1)) return -1;
    d->in_block = m->blocknum + 1;  // only this thread moves blocknum (below, once the transform is done)
  }
  if (d->fetch(m->fdomain, (m->in_type == REAL) ? N / 2 + 1 : N)) return -1;

  pthread_mutex_lock(&m->filter_mutex);  // filter.c:154-157
  m->blocknum++;
  pthread_cond_broadcast(&m->filter_cond);
  pthread_mutex_unlock(&m->filter_mutex);

  if (m->in_type == REAL)
    memmove(m->input_buffer.r, m->input_buffer.r + m->ilen, (m->impulse_length - 1) * sizeof(float));
  else
    memmove(m->input_buffer.c, m->input_buffer.c + m->ilen, (m->impulse_length - 1) * sizeof(kq_cfloat));
  return 0;
}

int delete_filter_input(struct filter_in *m) {
  if (m == NULL) return 0;
  CompatScope dev_scope_;
  MasterDev *d = (MasterDev *)m->fwd_plan;
  if (d) {
    d->close();
    delete d;
  }
  free(m->input_buffer.c);  // same storage either way (union), as filter.c:259
  free(m->fdomain);
  free(m);
  return 0;
}

float noise_gain(struct filter_out const *f) {
  if (f == NULL) return NAN;
  struct filter_in const *m = f->master;
  int const N = (int)(m->ilen + m->impulse_length - 1);
  int const nd = N / (int)f->decimate;
  int const count = (m->in_type == REAL && f->out_type == REAL) ? nd / 2 + 1 : nd;
  float sum = 0;
  for (int i = 0; i < count; i++) sum += re(f->response[i]) * re(f->response[i]) + im(f->response[i]) * im(f->response[i]);
  if (f->out_type == REAL || f->out_type == CROSS_CONJ) return 2 * N * sum;
  return N * sum;
}

struct filter_out *create_filter_output(struct filter_in *master, kq_cfloat *response, unsigned int decimate,
                                        enum filtertype out_type) {
  if (master == NULL || decimate == 0) return NULL;  // filter.c:99-100
  CompatScope dev_scope_;
  int const N = (int)(master->ilen + master->impulse_length - 1);
  int const nd = N / (int)decimate;
  if ((N % decimate) != 0) fprintf(stderr, "Warning: FFT size %d is not divisible by decimation ratio %u\n", N, decimate);
  {
    bool dim_ok = false;
    if (nd >= 4 && nd <= 16384) (void)kq::fft_dim(nd, &dim_ok);  // (makes and caches the plan the slave's kernel will ask for)
    if (!dim_ok) {
      fprintf(stderr, "ka9q_hip: create_filter_output: N/decimate=%d must be an even 2^a 3^b 5^c 7^d in 4..16384\n", nd);
      return NULL;
    }
  }
  struct filter_out *s = (struct filter_out *)calloc(1, sizeof(*s));
  if (!s) return NULL;
  pthread_mutex_init(&s->response_mutex, NULL);
  s->master = master;
  s->out_type = out_type;
  s->decimate = decimate;
  s->olen = master->ilen / decimate;
  s->response = response;
  s->noise_gain = response ? noise_gain(s) : NAN;
  SlaveDev *d = new SlaveDev();
  s->rev_plan = d;
  d->Ndec = nd;
  if (d->open_stream(ctx().stream) || d->alloc(&d->d_resp, nd, true) || d->alloc(&d->d_out, nd)) {
    s->response = NULL;  // (still the caller's)
    delete_filter_output(s);
    return NULL;
  }
  if (out_type == REAL) {
    s->output_buffer.r = (float *)calloc(nd, sizeof(float));
    s->output.r = s->output_buffer.r + nd - s->olen;  // filter.c:140
  } else {
    s->output_buffer.c = (kq_cfloat *)calloc(nd, sizeof(kq_cfloat));
    s->output.c = s->output_buffer.c + nd - s->olen;  // filter.c:131
  }
  return s;
}

int execute_filter_output(struct filter_out *s) {
  if (s == NULL) return -1;
  CompatScope dev_scope_;
  struct filter_in *m = s->master;
  MasterDev *md = (MasterDev *)m->fwd_plan;
  SlaveDev *sd = (SlaveDev *)s->rev_plan;
  hipStream_t st = sd->stream;

  pthread_mutex_lock(&m->filter_mutex);  // filter.c:195-199: wait for a new block
  while (s->blocknum == m->blocknum) pthread_cond_wait(&m->filter_cond, &m->filter_mutex);
  s->blocknum = m->blocknum;
  pthread_mutex_unlock(&m->filter_mutex);

  int const nd = sd->Ndec;
  bool const real_out = s->out_type == REAL;
  // REAL in / REAL out reads N_dec/2+1 response bins (filter.c:209-212); every other combination reads all N_dec,
  // COMPLEX in / REAL out included: it folds in H[N_dec - p] X[N - p] (filter.c:232-234).  The same rule as noise_gain().
  size_t const rbins = (real_out && m->in_type == REAL) ? nd / 2 + 1 : nd;
  pthread_mutex_lock(&s->response_mutex);  // filter.c:201
  if (s->response == NULL) {
    pthread_mutex_unlock(&s->response_mutex);
    return -1;
  }
  hipError_t e = hipMemcpyAsync(sd->d_resp, s->response, rbins * sizeof(float2), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  pthread_mutex_unlock(&s->response_mutex);
  if (e != hipSuccess) return -1;

  kq::launch_slave_single(st, md->d_out, sd->d_resp, sd->d_out, md->n, nd, m->in_type == REAL, (int)s->out_type, md->tw,
                          md->log2T);
  size_t const obytes = real_out ? nd * sizeof(float) : nd * sizeof(float2);
  if (hipMemcpyAsync(s->output_buffer.c, sd->d_out, obytes, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  return 0;
}

int delete_filter_output(struct filter_out *s) {
  if (s == NULL) return 0;
  CompatScope dev_scope_;
  SlaveDev *d = (SlaveDev *)s->rev_plan;
  if (d) {
    d->close();
    delete d;
  }
  pthread_mutex_destroy(&s->response_mutex);
  free(s->output_buffer.c);
  free(s->response);
  free(s);
  return 0;
}

int make_kaiser(float *window, unsigned int M, float beta) {
  if (window == NULL) return -1;
  if (!ctx_init()) return -1;
  CompatScope dev_scope_;
  return kq::make_kaiser(window, M, beta);
}

int window_filter(int L, int M, kq_cfloat *response, float beta) {
  if (response == NULL) return -1;
  if (!ctx_init()) return -1;
  CompatScope dev_scope_;
  int const N = L + M - 1;
  std::vector<kq::cfloat> r(N);
  memcpy((void *)r.data(), response, N * sizeof(kq_cfloat));
  if (kq::window_filter(L, M, r, beta)) return -1;
  memcpy(response, r.data(), N * sizeof(kq_cfloat));
  return 0;
}

int window_rfilter(int L, int M, kq_cfloat *response, float beta) {
  if (response == NULL) return -1;
  if (!ctx_init()) return -1;
  CompatScope dev_scope_;
  int const N = L + M - 1;
  std::vector<kq::cfloat> r(N / 2 + 1);
  memcpy((void *)r.data(), response, r.size() * sizeof(kq_cfloat));
  if (kq::window_rfilter(L, M, r, beta)) return -1;
  memcpy(response, r.data(), r.size() * sizeof(kq_cfloat));
  return 0;
}

int set_filter(struct filter_out *s, float low, float high, float kaiser_beta) {
  if (s == NULL) return -1;
  if (std::isnan(low) || std::isnan(high)) return -1;  // filter.c:504-505
  struct filter_in *m = s->master;
  int const L_dec = (int)s->olen;
  int const M_dec = (int)((m->impulse_length - 1) / s->decimate + 1);
  int const N = (int)(m->ilen + m->impulse_length - 1);
  CompatScope dev_scope_;
  std::vector<kq::cfloat> r = kq::design_response(N, L_dec, M_dec, (int)s->out_type, low, high, kaiser_beta);
  if (r.empty()) return -1;
  kq_cfloat *fresh = (kq_cfloat *)malloc(r.size() * sizeof(kq_cfloat));
  if (!fresh) return -1;
  memcpy(fresh, r.data(), r.size() * sizeof(kq_cfloat));
  pthread_mutex_lock(&s->response_mutex);  // hot swap: filter.c:538-543
  kq_cfloat *old = s->response;
  s->response = fresh;
  s->noise_gain = noise_gain(s);
  pthread_mutex_unlock(&s->response_mutex);
  free(old);
  return 0;
}

}  // extern "C"
