// kq_compat_osc.cpp -- the host arithmetic of the compat surface (include/ka9q_hip_compat.h): the scalar oscillator of
// osc.h:21-24, dsp.h's csincos* and cnrm*, and the notch filter of filter.c:551-571.  No device, no HIP: plain C++.
#include <cmath>
#include <cstdlib>

#include "../../include/ka9q_hip_compat.h"

extern "C" {

// ---- NCO (host scalar API; inside the bank the kernels evaluate the same sequence in closed form) ----
int is_phasor_init(kq_cdouble x) {
  double const a = __real__ x, b = __imag__ x;
  if (std::isnan(a) || std::isnan(b) || a * a + b * b < 0.9) return 0;  // osc.c:14-18
  return 1;
}

static kq_cdouble unit_pi(double x) {
  kq_cdouble z;
  __real__ z = std::cos(x * M_PI);
  __imag__ z = std::sin(x * M_PI);
  return z;
}

void set_osc(struct osc *o, double f, double r) {
  pthread_mutex_lock(&o->mutex);
  if (!is_phasor_init(o->phasor)) {  // osc.c:24-27
    __real__ o->phasor = 1;
    __imag__ o->phasor = 0;
    o->steps = 0;
  }
  o->freq = f;
  o->rate = r;
  o->phasor_step = unit_pi(2 * f);
  if (r != 0) {
    o->phasor_step_step = unit_pi(2 * r);
  } else {
    __real__ o->phasor_step_step = 1;
    __imag__ o->phasor_step_step = 0;
  }
  pthread_mutex_unlock(&o->mutex);
}

static inline kq_cdouble zmul(kq_cdouble a, kq_cdouble b) {
  kq_cdouble z;
  __real__ z = __real__ a * __real__ b - __imag__ a * __imag__ b;
  __imag__ z = __real__ a * __imag__ b + __imag__ a * __real__ b;
  return z;
}

void renorm_osc(struct osc *o) {
  o->steps = 0;
  double const mag = std::hypot(__real__ o->phasor, __imag__ o->phasor);
  __real__ o->phasor /= mag;
  __imag__ o->phasor /= mag;
  if (o->rate != 0) {
    double const ms = std::hypot(__real__ o->phasor_step, __imag__ o->phasor_step);
    __real__ o->phasor_step /= ms;
    __imag__ o->phasor_step /= ms;
  }
}

kq_cdouble step_osc(struct osc *o) {
  kq_cdouble const now = o->phasor;
  if (o->freq != 0) {  // osc.c:43-47
    o->phasor = zmul(o->phasor, o->phasor_step);
    if (o->rate != 0) o->phasor_step = zmul(o->phasor_step, o->phasor_step_step);
  }
  if (++o->steps == 16384) renorm_osc(o);  // Renorm_rate, osc.c:11
  return now;
}

// ---- dsp.h helpers ----
kq_cfloat csincosf(float x) {
  kq_cfloat z;
  __real__ z = cosf(x);
  __imag__ z = sinf(x);
  return z;
}
kq_cfloat csincospif(float x) { return csincosf(x * (float)M_PI); }
kq_cdouble csincos(double x) {
  kq_cdouble z;
  __real__ z = std::cos(x);
  __imag__ z = std::sin(x);
  return z;
}
kq_cdouble csincospi(double x) { return csincos(x * M_PI); }
// filter.c:551-571.  Mixed float/double complex arithmetic as C evaluates it: the products with the double phasor
// are formed in double and rounded to float on assignment.
struct notchfilter *notch_create(double f, float bw) {
  struct notchfilter *nf = (struct notchfilter *)calloc(1, sizeof(struct notchfilter));
  if (!nf) return nullptr;
  __real__ nf->osc_phase = 1;
  __imag__ nf->osc_phase = 0;
  nf->osc_step = csincospi(2 * f);
  __real__ nf->dcstate = 0;
  __imag__ nf->dcstate = 0;
  nf->bw = bw;
  return nf;
}

kq_cfloat notch(struct notchfilter *nf, kq_cfloat s) {
  kq_cfloat r;
  if (!nf) {
    __real__ r = NAN;
    __imag__ r = 0;
    return r;
  }
  double const pr = __real__ nf->osc_phase, pi = __imag__ nf->osc_phase;
  double const sr = __real__ s, si = __imag__ s;
  // s = s * conj(osc_phase) - dcstate
  float const dr = (float)((sr * pr + si * pi) - (double)__real__ nf->dcstate);
  float const di = (float)((si * pr - sr * pi) - (double)__imag__ nf->dcstate);
  // dcstate += bw * s
  __real__ nf->dcstate = __real__ nf->dcstate + nf->bw * dr;
  __imag__ nf->dcstate = __imag__ nf->dcstate + nf->bw * di;
  // s *= osc_phase
  __real__ r = (float)((double)dr * pr - (double)di * pi);
  __imag__ r = (float)((double)dr * pi + (double)di * pr);
  // osc_phase *= osc_step
  double const tr = __real__ nf->osc_step, ti = __imag__ nf->osc_step;
  __real__ nf->osc_phase = pr * tr - pi * ti;
  __imag__ nf->osc_phase = pr * ti + pi * tr;
  return r;
}

float cnrmf(kq_cfloat x) { return __real__ x * __real__ x + __imag__ x * __imag__ x; }
double cnrm(kq_cdouble x) { return __real__ x * __real__ x + __imag__ x * __imag__ x; }

}  // extern "C"
