// kq_fmstage.hpp -- what every compiled form of the demodulators writes the same way: the n0 smoother's step and the FM
// status record (kq_demod64.hip: the one-wave pair and the four-wave pipeline; kq_demod_fm.hip: k_demod_fm, k_demod_fm256).
#pragma once
#include "kq_device.hpp"

namespace kq {

// one block's step of the smoothed noise density (fm.c:79-82, am.c:46-49); the reference's rate is a double literal
__device__ __forceinline__ float n0_step(float n0, float fresh, double rate) {
  return isnan(n0) ? fresh : (float)((double)n0 + rate * (double)(fresh - n0));
}

// an FM block's record; n0: NaN where compute_n0 is off.  plfreq is NaN until k_pl_track fills it in (N/D = 64: the PL slave
// would have 2 points, fm.c:203, measurement off)
__device__ __forceinline__ kq_chan_status fm_status_record(float if_power, float noise_gain, float n0, float bb_power, float snr,
                                                           float foffset, float pdeviation, int squelch_count, int blanked,
                                                           int nout) {
  kq_chan_status st;
  st.if_power = if_power;
  st.noise_gain = noise_gain;
  st.plfreq = NAN;
  st.cphase = 0;
  st.pll_lock = 0;
  st.lock_count = 0;
  st.n0 = n0;
  st.bb_power = bb_power;
  st.snr = snr;
  st.foffset = foffset;
  st.pdeviation = pdeviation;
  st.agc_gain = 0;
  st.squelch_count = squelch_count;
  st.hangcount = 0;
  st.blanked = blanked;
  st.nout = nout;
  return st;
}

}  // namespace kq
