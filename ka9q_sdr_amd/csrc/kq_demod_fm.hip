// kq_demod_fm.hip -- the FM demodulator for any geometry (fm.c; N/D = 64: kq_demod64.hip).
//
//   k_demod_fm          amplitude statistics, squelch, discriminator, offset / deviation, status records
//   k_fm_audio          de-emphasis overlap-save and PL slave, one workgroup per (channel, block)
//   k_fm_audio256       the same for N/D = 256 with the PL measurement on: one wave per pair of blocks, in registers
//   k_demod_fm256       the whole demodulator of N/D = 256 without the PL measurement in one launch; Audio256 is its form of
//                       k_fm_audio256's transform pair (the same values to rounding, not to the bit: DESIGN_DIARY.md)
//   fm_disc_waves, fm_disc_lds_bytes, fm_audio_lds_bytes, demod_fm_lds_bytes: the dynamic-LDS carves
//   k_pl_track          PL tone tracker on the slave's output (fm.c:236-277)
//   launch_demod_fm picks among the three forms; launch_pl_track follows it where the measurement is on.
#include <algorithm>

#include "kq_device.hpp"
#include "kq_fmstage.hpp"
#include "kq_ldsfft.hpp"

namespace kq {

// FM, generic geometry, in two kernels.
//   k_demod_fm   amplitude statistics, squelch, discriminator with the hold rule, frequency offset / deviation
//                (fm.c:91-160); the detected samples of every block go to `fmout`.
//   k_fm_audio   the REAL->REAL de-emphasis overlap-save and the PL slave (fm.c:162-171, 219-234), one wave per
//                (channel, block).
// k_demod_fm.  fm.c walks the blocks of a channel in sequence, but what one block hands to the next is small: the
// squelch counter, the last strong sample (conjugated) and the last good audio value, and the offset / deviation
// readings that are only refreshed while the squelch is fully open.  So a workgroup takes one channel and 64 blocks
// at a time in four phases, with W waves sharing the blocks in the two heavy ones:
//   A  (per block)   amplitude statistics -> bb, snr, threshold; the last two strong samples of the block
//   B  (wave 0)      lanes = blocks: squelch counters from the snr flags; for every block the state and audio value it
//                    starts from, found at the nearest earlier block that defines them (squelched: zeros; open with a
//                    strong sample: that sample and its discriminator output)
//   C  (per block)   discriminator, hold rule, sums -> fmout and the block's own offset / deviation
//   D  (wave 0)      lanes = blocks: offset / deviation carried from the nearest block that measured them, the n0
//                    smoother, status records
// Every per-block expression and reduction order is that of the sequential loop, so results do not depend on W.
// Dynamic LDS: per wave  S float2[olen] | Y float[olen].
namespace {
__device__ __forceinline__ int top_bit(unsigned long long m) { return 63 - __clzll((long long)m); }
__device__ __forceinline__ unsigned long long bits_upto(int k) { return (2ull << k) - 1ull; }   // bits 0..k
__device__ __forceinline__ unsigned long long bits_below(int k) { return (1ull << k) - 1ull; }  // bits 0..k-1

// ---- what k_demod_fm and k_demod_fm256 (below: the same four phases with the call's blocks held in LDS) share
// per-block records of the current 64-block chunk; each kernel has one in LDS
struct FmChunk {
  float r_bb[64], r_snr[64], r_amp[64], r_la_out[64], r_la_in[64], r_foff[64], r_pdev[64];
  int r_carry[64], r_pvc[64], r_sq[64], r_blanked[64];
  float2 r_sc[64], r_sp[64], r_st_out[64], r_st_in[64];
};
// carried from block to block (fm.c:26,68-69 and struct demod); only wave 0 uses them
struct FmCarried {
  float2 c_state;
  float c_la;
  int c_sq;
  float c_foff, c_pdev, c_n0;
  __device__ __forceinline__ void load(const ChanDev &ch, int c) {
    c_state = ch.fm_state[c];
    c_la = ch.lastaudio[c];
    c_sq = ch.sq_count[c];
    c_foff = ch.foffset[c], c_pdev = ch.pdev[c];
    c_n0 = ch.n0[c];
  }
  __device__ __forceinline__ void store(const ChanDev &ch, int c) const {
    ch.n0[c] = c_n0;
    ch.fm_state[c] = c_state;
    ch.lastaudio[c] = c_la;
    ch.sq_count[c] = c_sq;
    ch.foffset[c] = c_foff;
    ch.pdev[c] = c_pdev;
  }
};

// phase A's tail: a block's statistics from its two sums (fm.c:99-103) and the blanking threshold (fm.c:121)
__device__ __forceinline__ float fm_threshold(float amp) { return (float)(0.55 * 0.55 * amp * amp); }
struct FmBlockStats {
  float bb, amp, snr, thr;
};
__device__ __forceinline__ FmBlockStats fm_block_stats(float sum_t, float sum_a, int olen) {
  FmBlockStats r;
  r.bb = sum_t / (2 * olen);
  r.amp = (float)((double)sum_a / (M_SQRT2 * olen));
  float const variance = r.bb - r.amp * r.amp;
  float snr = r.amp * r.amp / (2 * variance) - 1;
  r.snr = (0.0f > snr) ? 0.0f : snr;  // misc.h max(): NaN propagates
  r.thr = fm_threshold(r.amp);
  return r;
}
// ... and its record, by lane 0; carry, pvc: the block's last strong sample and the one before it (-1: none), S: its samples
__device__ __forceinline__ void fm_record_stats(FmChunk &rec, int k, const FmBlockStats &st, int carry, int pvc, const float2 *S) {
  rec.r_bb[k] = st.bb;
  rec.r_snr[k] = st.snr;
  rec.r_amp[k] = st.amp;
  rec.r_carry[k] = carry;
  rec.r_pvc[k] = pvc;
  rec.r_sc[k] = carry >= 0 ? S[carry] : make_float2(0.f, 0.f);
  rec.r_sp[k] = pvc >= 0 ? S[pvc] : make_float2(0.f, 0.f);
}

// phase B (wave 0, lanes = blocks): squelch counters and what every block starts from
__device__ __forceinline__ void fm_phase_b(FmChunk &rec, FmCarried &cr, int nb) {
  int const lane = threadIdx.x & 63;
  bool const act = lane < nb;
  bool const reset = act && rec.r_snr[lane] > 2;  // fm.c:108-114
  unsigned long long const rm = __ballot(reset), rl = rm & bits_upto(lane);
  int const sq = rl ? lane - top_bit(rl) : min(cr.c_sq + lane + 1, 1000);
  bool const open = sq < 2;
  int const carry = act ? rec.r_carry[lane] : -1;
  // a squelched block leaves zeros behind (fm.c:156-160), an open one with a strong sample leaves that sample
  bool const def = act && (!open || carry >= 0);
  float2 const sc = rec.r_sc[lane];
  rec.r_st_out[lane] = open ? cconj(sc) : make_float2(0.f, 0.f);
  unsigned long long const dm = __ballot(def), dl = dm & bits_below(lane);
  int const j = dl ? top_bit(dl) : -1;
  wave_sync();
  float2 const st_in = j >= 0 ? rec.r_st_out[j] : cr.c_state;
  float ylast = 0;
  if (open && carry >= 0) {  // the discriminator output at the block's last strong sample (fm.c:130-132)
    float2 const st = rec.r_pvc[lane] >= 0 ? cconj(rec.r_sp[lane]) : st_in;
    float2 const pr = cmul(sc, st);
    ylast = atan2f(pr.y, pr.x);
  }
  rec.r_la_out[lane] = ylast;
  wave_sync();
  rec.r_la_in[lane] = j >= 0 ? rec.r_la_out[j] : cr.c_la;
  rec.r_st_in[lane] = st_in;
  rec.r_sq[lane] = sq;
  if (dm) {
    int const jl = top_bit(dm);
    cr.c_state = rec.r_st_out[jl];
    cr.c_la = rec.r_la_out[jl];
  }
  cr.c_sq = __shfl(sq, nb - 1, 64);
}

// phase C, one block by one wave: discriminator and hold rule (fm.c:116-160).  S: the block's samples, Y: the wave's
// discriminator outputs before the hold, fo: where the detected samples go.  OLEN = 0: any block length, olen samples;
// otherwise the length itself, a multiple of 64 (no lane is ever past the block's end).  The wave's lane 0 records the result.
struct FmBlockReadings {
  int blanked;
  float foff, pdev;
};
template <int OLEN>
__device__ __forceinline__ FmBlockReadings fm_block_discriminate(const Geom &g, const float2 *S, float *Y, float *fo, int olen_any,
                                                                 float thr, float2 st_in, float la_in, int sq) {
  static_assert(OLEN % 64 == 0, "whole groups of 64 samples");
  int const lane = threadIdx.x & 63;
  int const olen = OLEN ? OLEN : olen_any;
  auto const inside = [&](int n) { return OLEN != 0 || n < olen; };
  FmBlockReadings r = {0, 0.f, 0.f};
  if (sq >= 2) {
    for (int n = lane; n < olen; n += 64) fo[n] = 0;  // fm.c:156-160
    return r;
  }
  int carry = -1;
  for (int cb = 0; cb < olen; cb += 64) {
    int const n = cb + lane;
    float2 const v = S[inside(n) ? n : 0];
    bool const valid = inside(n) && cnrm(v) > thr;
    unsigned long long const m = __ballot(valid), ml = m & bits_below(lane);
    if (valid) {  // arg(s_n * conj(previous strong sample)), fm.c:130-132
      int const pv = ml ? cb + top_bit(ml) : carry;
      float2 const st = pv >= 0 ? cconj(S[pv]) : st_in;
      float2 const pr = cmul(v, st);
      Y[n] = atan2f(pr.y, pr.x);
    }
    if (m) carry = cb + top_bit(m);
  }
  wave_sync();
  // weak samples repeat the last good audio value (fm.c:141)
  float sum_y = 0, vmax = -INFINITY, vmin = INFINITY;
  bool first_valid = false;
  carry = -1;
  for (int cb = 0; cb < olen; cb += 64) {
    int const n = cb + lane;
    bool const valid = inside(n) && cnrm(S[inside(n) ? n : 0]) > thr;
    unsigned long long const m = __ballot(valid), mu = m & bits_upto(lane);
    if (cb == 0) first_valid = (m & 1ull) != 0;
    if (inside(n)) {
      int const lv = mu ? cb + top_bit(mu) : carry;
      float const y = lv >= 0 ? Y[lv] : la_in;
      fo[n] = y;
      sum_y += y;
      if (valid) {
        if (n > 0) {
          vmax = fmaxf(vmax, y);
          vmin = fminf(vmin, y);
        }
      } else {
        r.blanked++;
      }
    }
    if (m) carry = cb + top_bit(m);
  }
  sum_y = wave_sum(sum_y);
  vmax = wave_max(vmax);
  vmin = wave_min(vmin);
  r.blanked = wave_sum_i(r.blanked);
  // peak-deviation seeds: sample 0 seeds both only when it is strong (fm.c:125-139)
  float const seed = first_valid ? Y[0] : 0.0f;
  float pdev_pos = fmaxf(seed, vmax), pdev_neg = fminf(seed, vmin);
  float const avg_f = sum_y / olen;
  if (sq < 1) {  // fm.c:146-154
    r.foff = (float)(g.dsamprate * avg_f * (0.5 * M_1_PI));
    pdev_pos -= avg_f;
    pdev_neg -= avg_f;
    float const mx = (pdev_pos > -pdev_neg) ? pdev_pos : -pdev_neg;
    r.pdev = (float)(g.dsamprate * mx * (0.5 * M_1_PI));
  }
  wave_sync();  // Y (and S, where it is the wave's own) is reused by this wave's next block
  return r;
}

// phase D (wave 0, lanes = blocks): carried readings, the n0 smoother and the status records of blocks b0 .. b0 + nb - 1
__device__ __forceinline__ void fm_phase_d(const FmChunk &rec, FmCarried &cr, const Geom &g, const Planes &pl, int c, int b0, int nb,
                                           float noise_gain, int compute_n0, int olen) {
  int const lane = threadIdx.x & 63;
  bool const act = lane < nb;
  int const sq = rec.r_sq[lane];
  bool const own = act && sq < 1;
  unsigned long long const om = __ballot(own), ol = om & bits_upto(lane);
  int const jo = ol ? top_bit(ol) : -1;
  float const foffset = jo >= 0 ? rec.r_foff[jo] : cr.c_foff;
  float const pdev = jo >= 0 ? rec.r_pdev[jo] : cr.c_pdev;
  if (om) {
    int const jl = top_bit(om);
    cr.c_foff = rec.r_foff[jl];
    cr.c_pdev = rec.r_pdev[jl];
  }
  float n0_mine = NAN;
  if (compute_n0) {  // fm.c:79-82: a chain in double through the blocks
    float const fresh_v = act ? pl.n0raw[(size_t)c * g.max_blocks + b0 + lane] : 0.f;
    for (int k = 0; k < nb; k++) {
      float const fresh = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fresh_v), k));
      cr.c_n0 = n0_step(cr.c_n0, fresh, .01);
      if (lane == k) n0_mine = cr.c_n0;
    }
  }
  if (act)
    pl.status[(size_t)c * g.max_blocks + b0 + lane] =
        fm_status_record(pl.if_power[b0 + lane], noise_gain, n0_mine, rec.r_bb[lane], rec.r_snr[lane], foffset, pdev, sq,
                         rec.r_blanked[lane], olen);
}
}  // namespace

__global__ void __launch_bounds__(1024) k_demod_fm(Geom g, ChanDev ch, Planes pl, float *__restrict__ fmout,
                                                   const int *__restrict__ list, int nblocks, int compute_n0) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ FmChunk rec;
  int const c = list[blockIdx.x];
  int const lane = threadIdx.x & 63;
  int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  int const olen = g.olen;
  float2 *S = lds + (size_t)wave * olen;
  float *Y = reinterpret_cast<float *>(lds + (size_t)W * olen) + (size_t)wave * olen;
  FmCarried cr;
  cr.load(ch, c);
  float const noise_gain = ch.noise_gain[c];

  for (int b0 = 0; b0 < nblocks; b0 += 64) {
    int const nb = min(64, nblocks - b0);
    // ---- A: amplitude statistics (fm.c:91-103) and the last two strong samples of each block
    for (int k = wave; k < nb; k += W) {
      const float2 *in = pl.filt + ((size_t)c * g.max_blocks + b0 + k) * olen;
      float sum_t = 0, sum_a = 0;
      for (int n = lane; n < olen; n += 64) {
        float2 const v = in[n];
        S[n] = v;
        float const t = cnrm(v);
        sum_t += t;
        sum_a += sqrtf(t);
      }
      sum_t = wave_sum(sum_t);
      sum_a = wave_sum(sum_a);
      FmBlockStats const st = fm_block_stats(sum_t, sum_a, olen);
      int carry = -1, pvc = -1;  // last strong sample and the one before it
      for (int cb = 0; cb < olen; cb += 64) {
        int const n = cb + lane;
        bool const valid = n < olen && cnrm(S[n < olen ? n : 0]) > st.thr;
        unsigned long long const m = __ballot(valid);
        if (m) {
          int const top = top_bit(m);
          unsigned long long const rest = m & ~(1ull << top);
          pvc = rest ? cb + top_bit(rest) : carry;
          carry = cb + top;
        }
      }
      wave_sync();
      if (lane == 0) fm_record_stats(rec, k, st, carry, pvc, S);
      wave_sync();
    }
    __syncthreads();
    // ---- B: squelch counters and what every block starts from
    if (wave == 0) fm_phase_b(rec, cr, nb);
    __syncthreads();
    // ---- C: discriminator and hold rule (fm.c:116-160)
    for (int k = wave; k < nb; k += W) {
      const float2 *in = pl.filt + ((size_t)c * g.max_blocks + b0 + k) * olen;
      float *fo = fmout + ((size_t)c * g.max_blocks + b0 + k) * olen;
      int const sq = rec.r_sq[k];
      if (sq < 2) {
        for (int n = lane; n < olen; n += 64) S[n] = in[n];
        wave_sync();
      }
      FmBlockReadings const r = fm_block_discriminate<0>(g, S, Y, fo, olen, fm_threshold(rec.r_amp[k]), rec.r_st_in[k], rec.r_la_in[k], sq);
      if (lane == 0) {
        rec.r_blanked[k] = r.blanked;
        rec.r_foff[k] = r.foff;
        rec.r_pdev[k] = r.pdev;
      }
    }
    __syncthreads();
    // ---- D: carried readings and the status records
    if (wave == 0) fm_phase_d(rec, cr, g, pl, c, b0, nb, noise_gain, compute_n0, olen);
    __syncthreads();
  }
  if (threadIdx.x == 0) cr.store(ch, c);
}

// De-emphasis overlap-save and PL slave of one (channel, block): REAL -> REAL (fm.c:162-171, 219-234;
// filter.c:151,206-208,250).  The filter input is the channel's stream of detected samples: `hist_in` holds the
// AM-1 samples that precede block 0 of this call, `fmout` the blocks of the call.  The workgroup of the last block
// writes the AM-1 samples that will precede the next call into `hist_out` (a different buffer: every block-0
// workgroup of this launch is still reading hist_in).
// Dynamic LDS carve:  F float2[AN] | AIN float[AN] | PLB float2[pl_n] | TWL float2[AN/2]
__global__ void __launch_bounds__(256) k_fm_audio(Geom g, ChanDev ch, Planes pl, const float2 *__restrict__ tw,
                                                 const float *__restrict__ fmout, const float *__restrict__ hist_in,
                                                 float *__restrict__ hist_out, const int *__restrict__ list, int nblocks) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int const c = list[blockIdx.x], b = blockIdx.y;
  int const lane = threadIdx.x, nthr = blockDim.x;  // 64 ... 256 threads (launch_demod_fm): every loop strides by the workgroup
  int const AN = g.Ndec, AM = g.Mdec, AL = g.olen;
  float2 *F = lds;
  float *AIN = reinterpret_cast<float *>(F + AN);
  float2 *PLB = reinterpret_cast<float2 *>(AIN + AN);
  float2 *TWL = PLB + g.pl_n;  // exp(-2 pi i k / AN), k < AN/2
  // AN with a factor 3, 5 or 7 (kq_ldsfft.hpp lds_fft_mixed): twiddles from the plan's own table; where TWL would sit, a second
  // buffer of AN bins takes the products in digit-reversed order (that permutation is no involution: no swapping in place)
  bool const mixed = g.dNdec.log2n < 0;
  float2 *F2 = TWL;
  bool const pl_on = g.pl_n > 0 && pl.plout != nullptr;
  bool const flat = (ch.flags[c] & FLAG_FLAT) != 0;
  const float *stream = fmout + (size_t)c * g.max_blocks * AL;  // detected samples of this call, block after block
  const float *hin = hist_in + (size_t)c * (AM - 1);
  // sample j of the stream, j >= -(AM-1)
  auto sample = [&](long long j) { return j >= 0 ? stream[j] : hin[(AM - 1) + j]; };
  if (b == nblocks - 1) {
    float *ho = hist_out + (size_t)c * (AM - 1);
    for (int i = lane; i < AM - 1; i += nthr) ho[i] = sample((long long)nblocks * AL - (AM - 1) + i);
  }
  float *aud = pl.audio + ((size_t)c * g.max_blocks + b) * (2 * (size_t)AL);
  if (flat && !pl_on) {
    for (int n = lane; n < AL; n += nthr) aud[n] = stream[(size_t)b * AL + n];
    return;
  }
  if (!mixed)
    for (int k = lane; k < AN / 2; k += nthr) TWL[k] = tw[(size_t)k << (g.tw_log2 - g.log2Ndec)];
  for (int i = lane; i < AN; i += nthr) {
    float const v = sample((long long)b * AL - (AM - 1) + i);
    AIN[i] = v;
    F[fft_pos((unsigned)i, g.dNdec)] = make_float2(v, 0.f);
  }
  // forward transform of the audio master (fm.c:162, filter.c:151)
  if (mixed)
    lds_fft_mixed<-1>(F, g.dNdec);
  else
    lds_fft<-1>(F, g.log2Ndec, TWL, g.log2Ndec);
  if (pl_on) {
    // PL slave: REAL -> REAL, decimate 32 (fm.c:219,234; filter.c:206-208 then c2r of pl_n points)
    int const PN = g.pl_n;
    for (int k = lane; k <= PN / 2; k += nthr) {
      float2 gk = cmul(ch.plresp[k], F[k]);
      if (k == 0 || k == PN / 2) {
        gk.y = 0.f;
      } else {
        PLB[fft_pos((unsigned)(PN - k), g.dPl)] = cconj(gk);
      }
      PLB[fft_pos((unsigned)k, g.dPl)] = gk;
    }
    // by the slave's own plan, not the master's: floor(AN / 32) of an AN with a factor 3, 5 or 7 may be a power of two (270 -> 8,
    // 1050 -> 32), whose mixed plan has no stages.  TWL is filled for a power-of-two master only (F2 lies there otherwise), so
    // such a slave takes its few twiddles from the bank's half-circle table in memory
    if (g.dPl.log2n < 0)
      lds_fft_mixed<+1>(PLB, g.dPl);
    else if (mixed)
      lds_fft<+1>(PLB, g.dPl.log2n, tw, g.tw_log2);
    else
      lds_fft<+1>(PLB, g.dPl.log2n, TWL, g.log2Ndec);
    float *po = pl.plout + ((size_t)c * g.max_blocks + b) * g.pl_l;
    for (int n = lane; n < g.pl_l; n += nthr) po[n] = PLB[PN - g.pl_l + n].x;  // filter.c:140
    __syncthreads();
  }
  if (flat) {
    for (int n = lane; n < AL; n += nthr) aud[n] = AIN[AM - 1 + n];
    return;
  }
  // multiply DC..Nyquist (filter.c:206-208) and Hermitian-extend for the c2r transform, which ignores the
  // imaginary parts of DC and Nyquist.  Lane k touches only F[k] and F[AN-k].
  const float2 *HA = ch.aresp + (size_t)c * (AN / 2 + 1);
  if (mixed) {
    for (int k = lane; k <= AN / 2; k += nthr) {
      float2 const gk = cmul(HA[k], F[k]);
      if (k == 0 || k == AN / 2) {
        F2[fft_pos((unsigned)k, g.dNdec)] = make_float2(gk.x, 0.f);
      } else {
        F2[fft_pos((unsigned)k, g.dNdec)] = gk;
        F2[fft_pos((unsigned)(AN - k), g.dNdec)] = cconj(gk);
      }
    }
    lds_fft_mixed<+1>(F2, g.dNdec);
    float const gain = ch.fm_gain[c];
    for (int n = lane; n < AL; n += nthr) aud[n] = F2[AN - AL + n].x * gain;  // fm.c:169-170
    return;
  }
  for (int k = lane; k <= AN / 2; k += nthr) {
    float2 const gk = cmul(HA[k], F[k]);
    if (k == 0 || k == AN / 2) {
      F[k] = make_float2(gk.x, 0.f);
    } else {
      F[k] = gk;
      F[AN - k] = cconj(gk);
    }
  }
  __syncthreads();
  for (int i = lane; i < AN; i += nthr) {  // bit-reverse in place, then backward transform
    unsigned const r = bitrev((unsigned)i, g.log2Ndec);
    if (r > (unsigned)i) {
      float2 const t = F[i];
      F[i] = F[r];
      F[r] = t;
    }
  }
  lds_fft<+1>(F, g.log2Ndec, TWL, g.log2Ndec);
  float const gain = ch.fm_gain[c];
  for (int n = lane; n < AL; n += nthr) aud[n] = F[AN - AL + n].x * gain;  // fm.c:169-170
}

// The same de-emphasis overlap-save for AN = 256 (AL = 128, AM = 129: BASELINE cfg 2's geometry) with the PL measurement on
// (PL_N = 8, PL_L = 4; without it k_demod_fm256 does the whole demodulator): one wave per PAIR of blocks, registers and lane
// exchanges only (k_demod64's scheme for 64 points, four values per lane).
// The two real windows [b-1 | b] and [b | b+1] are the real and imaginary part of ONE complex 256-point sequence z; both are
// filtered by the same response, so Y0 + i Y1 = HAf . (W0 + i W1) = HAf . Z with HAf the response's Hermitian extension
// (real at DC and Nyquist, whose imaginary parts the c2r transform ignores, filter.c:250) -- no separation of the two
// spectra is needed -- and one inverse transform returns block b's audio as its real part, block b+1's as its imaginary part.
// 256 = 4 x 64: i = m + 64 a, k = 4 q + r (lane m, register a or r).  Forward, decimation in frequency: in-lane radix-4
// over a, twiddle W_256^{m r}, then four 64-point transforms across the lanes (natural in, bit-reversed out: lane l holds
// q = bitrev6(l)); inverse the other way round (bit-reversed in, natural out).  fm.c:162-171, filter.c:151,206-208,250.
__global__ void __launch_bounds__(64) k_fm_audio256(Geom g, ChanDev ch, Planes pl, const float *__restrict__ fmout,
                                                    const float *__restrict__ hist_in, float *__restrict__ hist_out,
                                                    const int *__restrict__ list, int nblocks) {
  constexpr int AL = 128, AN = 256;
  int const c = list[blockIdx.x], b0 = 2 * (int)blockIdx.y, lane = threadIdx.x;
  bool const have1 = b0 + 1 < nblocks;
  const float *stream = fmout + (size_t)c * g.max_blocks * AL;  // detected samples of this call, block after block
  const float *pm = b0 > 0 ? stream + (size_t)(b0 - 1) * AL : hist_in + (size_t)c * AL;  // AM - 1 = 128: exactly one block
  float const p0 = pm[lane], p1 = pm[lane + 64];
  float const c0 = stream[(size_t)b0 * AL + lane], c1 = stream[(size_t)b0 * AL + lane + 64];
  float const n0 = have1 ? stream[(size_t)(b0 + 1) * AL + lane] : 0.f, n1 = have1 ? stream[(size_t)(b0 + 1) * AL + lane + 64] : 0.f;
  if (b0 + 2 >= nblocks) {  // the call's last block precedes the next call (filter.c:164)
    float *ho = hist_out + (size_t)c * AL;
    ho[lane] = have1 ? n0 : c0;
    ho[lane + 64] = have1 ? n1 : c1;
  }
  float *aud0 = pl.audio + ((size_t)c * g.max_blocks + b0) * (2 * (size_t)AL);
  float *aud1 = aud0 + 2 * AL;
  bool const flat = (ch.flags[c] & FLAG_FLAT) != 0;
  if (flat) {  // fm.c:164-172: no filter, no gain (the PL slave below still runs)
    aud0[lane] = c0;
    aud0[lane + 64] = c1;
    if (have1) {
      aud1[lane] = n0;
      aud1[lane + 64] = n1;
    }
  }
  // response on this lane's four bins k = 4 bitrev6(lane) + r, Hermitian-extended
  const float2 *HA = ch.aresp + (size_t)c * (AN / 2 + 1);
  int const q = (int)(__brev((unsigned)lane) >> 26);
  float2 hf[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    int const k = 4 * q + r;
    float2 const t = HA[k <= AN / 2 ? k : AN - k];
    hf[r] = k <= AN / 2 ? t : cconj(t);
    if (k == 0 || k == AN / 2) hf[r].y = 0.f;
  }
  // lane-exchange twiddles of the 64-point transforms and the radix-4 twiddles W_256^{lane r}
  float2 wf[6], wi[6], w4[3];
#pragma unroll
  for (int s = 0; s < 6; s++) {
    int const half = 1 << s;
    float sn, cs;
    sincospif((float)(lane & (half - 1)) / (float)half, &sn, &cs);
    wf[s] = make_float2(cs, -sn);
    wi[s] = make_float2(cs, sn);
  }
#pragma unroll
  for (int r = 1; r < 4; r++) {
    float sn, cs;
    sincospif((float)(lane * r) / 128.f, &sn, &cs);
    w4[r - 1] = make_float2(cs, -sn);
  }
  auto xor_pow = [&](float2 v, int s) {
    switch (s) {
      case 0: return make_float2(lane_xor<1>(v.x, lane), lane_xor<1>(v.y, lane));
      case 1: return make_float2(lane_xor<2>(v.x, lane), lane_xor<2>(v.y, lane));
      case 2: return make_float2(lane_xor<4>(v.x, lane), lane_xor<4>(v.y, lane));
      case 3: return make_float2(lane_xor<8>(v.x, lane), lane_xor<8>(v.y, lane));
      case 4: return make_float2(lane_xor<16>(v.x, lane), lane_xor<16>(v.y, lane));
      default: return make_float2(lane_xor<32>(v.x, lane), lane_xor<32>(v.y, lane));
    }
  };
  auto muli = [](float2 a) { return make_float2(-a.y, a.x); };  // i a
  // z[m + 64 a]: real part the window [b0-1 | b0], imaginary part [b0 | b0+1]
  float2 const z0 = make_float2(p0, c0), z1 = make_float2(p1, c1), z2 = make_float2(c0, n0), z3 = make_float2(c1, n1);
  float2 u[4], xf[4];
  {
    float2 const t0 = cadd(z0, z2), t1 = csub(z0, z2), t2 = cadd(z1, z3), t3 = csub(z1, z3);
    u[0] = cadd(t0, t2);
    u[2] = cmul(csub(t0, t2), w4[1]);
    u[1] = cmul(csub(t1, muli(t3)), w4[0]);
    u[3] = cmul(cadd(t1, muli(t3)), w4[2]);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    float2 z = u[r];
#pragma unroll
    for (int s = 5; s >= 0; s--) {  // forward, decimation in frequency: natural in, bit-reversed out
      float2 const o = xor_pow(z, s);
      z = ((lane >> s) & 1) ? cmul(csub(o, z), wf[s]) : cadd(z, o);
    }
    xf[r] = z;           // X[4 bitrev6(lane) + r] of the pair's packed transform (the PL slave reads a few of them)
    z = cmul(hf[r], z);  // filter.c:206-208 on both windows at once
#pragma unroll
    for (int s = 0; s < 6; s++) {  // backward, decimation in time: bit-reversed in, natural out
      int const bit = (lane >> s) & 1;
      float2 const v = bit ? cmul(z, wi[s]) : z;
      float2 const o = xor_pow(v, s);
      z = bit ? csub(o, v) : cadd(v, o);
    }
    u[r] = r ? cmul(z, cconj(w4[r - 1])) : z;
  }
  {
    // PL slave of both blocks (fm.c:219,234: REAL -> REAL, decimate 32, 8 points, the last 4 kept): it needs bins 0..4 of each
    // window's own transform, W0[k] = (X[k] + conj X[256 - k]) / 2 and W1[k] = (X[k] - conj X[256 - k]) / 2i -- nine values
    // of the packed transform, held by lanes 0 (bins 0..3), 32 (bin 4) and 63 (bins 252..255).  Lane j < 8 forms output
    // n = 4 + (j & 3) of window j >> 2: y[n] = G0 + (-1)^n G4 + 2 Re sum_{k=1..3} G[k] e^{2 pi i k n / 8}, G = plresp . W.
    auto rd = [&](float2 v, int src) { return make_float2(__shfl(v.x, src, 64), __shfl(v.y, src, 64)); };
    float2 const X0 = rd(xf[0], 0), X1 = rd(xf[1], 0), X2 = rd(xf[2], 0), X3 = rd(xf[3], 0), X4 = rd(xf[0], 32);
    float2 const Xm1 = rd(xf[3], 63), Xm2 = rd(xf[2], 63), Xm3 = rd(xf[1], 63), Xm4 = rd(xf[0], 63);
    float2 const Xk[5] = {X0, X1, X2, X3, X4}, Xn[5] = {X0, Xm1, Xm2, Xm3, Xm4};
    int const w = (lane >> 2) & 1, n = 4 + (lane & 3);
    float y = 0.f;
#pragma unroll
    for (int k = 0; k <= 4; k++) {
      float2 const a = Xk[k], bc = cconj(Xn[k]);
      // window 0: (a + b) / 2; window 1: (a - b) / 2i = -i (a - b) / 2
      float2 const d = csub(a, bc);
      float2 const W = w ? make_float2(0.5f * d.y, -0.5f * d.x) : make_float2(0.5f * (a.x + bc.x), 0.5f * (a.y + bc.y));
      float2 gk = cmul(ch.plresp[k], W);
      if (k == 0 || k == 4) {
        y += (k == 4 && (n & 1)) ? -gk.x : gk.x;  // the c2r transform ignores the imaginary parts of DC and Nyquist
      } else {
        float sn, cs;
        sincospif((float)(k * n) * 0.25f, &sn, &cs);
        y += 2.f * (gk.x * cs - gk.y * sn);
      }
    }
    if (lane < 8 && (w == 0 || have1)) pl.plout[((size_t)c * g.max_blocks + b0 + w) * g.pl_l + (lane & 3)] = y;  // filter.c:140
    if (flat) return;
  }
  // inverse radix-4 over r, outputs i = 128 + m (a = 2) and 192 + m (a = 3) only: the samples the slave keeps (filter.c:140)
  float2 const y2 = csub(cadd(u[0], u[2]), cadd(u[1], u[3]));
  float2 const y3 = csub(csub(u[0], u[2]), muli(csub(u[1], u[3])));
  float const gain = ch.fm_gain[c];
  aud0[lane] = y2.x * gain;  // fm.c:169-170
  aud0[lane + 64] = y3.x * gain;
  if (have1) {
    aud1[lane] = y2.y * gain;
    aud1[lane + 64] = y3.y * gain;
  }
}

// The whole FM demodulator of one channel in ONE launch for N/D = 256 (cfg 2's geometry: 128 samples per block, de-emphasis
// filter of 129 taps) without the PL measurement: k_demod_fm's four phases and k_fm_audio256's overlap-save on the same
// 8-wave workgroup, the call's blocks held in LDS from the first load to the audio store.  What the two-kernel form pays
// and this does not: the second launch, the detected samples' round trip through memory (8 MB per call at cfg 2), and one
// exposed memory latency per block and phase -- a wave asks for all its blocks' samples at once here, and phase C finds
// them in LDS.  Per-block expressions and reduction orders are those of k_demod_fm / k_fm_audio256 (and so of the
// sequential loop of fm.c:91-171); the audio equals k_fm_audio256's to the last place or two (DESIGN_DIARY IV.14).
// Static LDS: S[64][128] float2 (64 KiB) | FO[65][128] float (row 0 = the block before the chunk) | Y[8][128] float.
namespace {
struct Audio256 {  // k_fm_audio256's transform pair, set up once per wave
  // wf / wi: the lane-exchange stages' twiddles as the lane applies them -- the stage's twiddle in the upper lane of a
  // butterfly pair, 1 in the lower one -- and sg: -1 / +1 likewise.  A stage is then the same six instructions in every
  // lane (round 6; until then both arms of `bit ? (o - z) w : z + o` were computed and one selected: twelve).  As written the
  // values are the old form's: o - z and z + o round once either way, and a product with (1, 0) is exact.  As compiled they
  // differ from k_fm_audio256's in the last place (DESIGN_DIARY IV.14), which is why that kernel keeps its own copy.
  float2 hf[4], wf[6], wi[6], w4[3];
  float sg[6];
  int lane;
  __device__ __forceinline__ void init(int lane_, const float2 *HA) {
    lane = lane_;
    int const q = (int)(__brev((unsigned)lane) >> 26);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      int const k = 4 * q + r;
      float2 const t = HA[k <= 128 ? k : 256 - k];
      hf[r] = k <= 128 ? t : cconj(t);
      if (k == 0 || k == 128) hf[r].y = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 6; s++) {
      int const half = 1 << s;
      float sn, cs;
      sincospif((float)(lane & (half - 1)) / (float)half, &sn, &cs);
      bool const up = (lane >> s) & 1;
      wf[s] = up ? make_float2(cs, -sn) : make_float2(1.f, 0.f);
      wi[s] = up ? make_float2(cs, sn) : make_float2(1.f, 0.f);
      sg[s] = up ? -1.f : 1.f;
    }
#pragma unroll
    for (int r = 1; r < 4; r++) {
      float sn, cs;
      sincospif((float)(lane * r) / 128.f, &sn, &cs);
      w4[r - 1] = make_float2(cs, -sn);
    }
  }
  // z[m + 64 a] = (window [b-1 | b], window [b | b+1]) -> the filtered samples 128 + m and 192 + m of both (real / imaginary part)
  __device__ __forceinline__ void run(float2 z0, float2 z1, float2 z2, float2 z3, float2 &y2, float2 &y3) const {
    auto muli = [](float2 a) { return make_float2(-a.y, a.x); };  // i a
    float2 u[4];
    {
      float2 const t0 = cadd(z0, z2), t1 = csub(z0, z2), t2 = cadd(z1, z3), t3 = csub(z1, z3);
      u[0] = cadd(t0, t2);
      u[2] = cmul(csub(t0, t2), w4[1]);
      u[1] = cmul(csub(t1, muli(t3)), w4[0]);
      u[3] = cmul(cadd(t1, muli(t3)), w4[2]);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float2 z = u[r];
#pragma unroll
      for (int s = 5; s >= 0; s--) {  // forward, decimation in frequency: upper lane (o - z) w, lower lane z + o
        float2 const o = lane_xor_pow2(z, s, lane);
        z = cmul(make_float2(fmaf(z.x, sg[s], o.x), fmaf(z.y, sg[s], o.y)), wf[s]);
      }
      z = cmul(hf[r], z);
#pragma unroll
      for (int s = 0; s < 6; s++) {  // backward, decimation in time: v = z w (upper) / z (lower); upper o - v, lower v + o
        float2 const v = cmul(z, wi[s]);
        float2 const o = lane_xor_pow2(v, s, lane);
        z = make_float2(fmaf(v.x, sg[s], o.x), fmaf(v.y, sg[s], o.y));
      }
      u[r] = r ? cmul(z, cconj(w4[r - 1])) : z;
    }
    y2 = csub(cadd(u[0], u[2]), cadd(u[1], u[3]));
    y3 = csub(csub(u[0], u[2]), muli(csub(u[1], u[3])));
  }
};
}  // namespace

// 8 waves per channel, two per SIMD (173 registers).  16 -- four per SIMD -- leave 128 registers, which spill 19 since the
// exchange stages of round 6, and measured no faster (three alternating rounds on one box: 35.3 / 35.2 / 35.7 us against
// 35.3 / 35.6 / 35.4 -- the launch is bound by its vector instruction count, 55 000 issue cycles per SIMD either way)
__global__ void __launch_bounds__(512) k_demod_fm256(Geom g, ChanDev ch, Planes pl, const float *__restrict__ hist_in,
                                                     float *__restrict__ hist_out, const int *__restrict__ list, int nblocks,
                                                     int compute_n0) {
  constexpr int olen = 128, W = 8;
  __shared__ __attribute__((aligned(16))) float2 S[64 * olen];
  __shared__ __attribute__((aligned(16))) float FO[65 * olen];
  __shared__ float Yall[W * olen];
  __shared__ FmChunk rec;
  int const c = list[blockIdx.x];
  int const lane = threadIdx.x & 63;
  int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *Y = Yall + wave * olen;
  FmCarried cr;
  cr.load(ch, c);
  float const noise_gain = ch.noise_gain[c];
  bool const flat = (ch.flags[c] & FLAG_FLAT) != 0;
  float const gain = ch.fm_gain[c];
  if (threadIdx.x < olen) FO[threadIdx.x] = hist_in[(size_t)c * olen + threadIdx.x];  // the block before the call (AM - 1 = 128)

  for (int b0 = 0; b0 < nblocks; b0 += 64) {
    int const nb = min(64, nblocks - b0);
    // ---- A: all of this wave's blocks asked for at once, then statistics block by block (fm.c:91-103)
    constexpr int kPer = 64 / W;
    float2 va[kPer], vb[kPer];
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      int const k = wave + W * i;
      if (k < nb) {
        const float2 *in = pl.filt + ((size_t)c * g.max_blocks + b0 + k) * olen;
        va[i] = in[lane];
        vb[i] = in[lane + 64];
      }
    }
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      int const k = wave + W * i;
      if (k >= nb) break;
      float2 *Sk = S + k * olen;
      Sk[lane] = va[i];
      Sk[lane + 64] = vb[i];
      float sum_t = 0, sum_a = 0;
      {  // (n = lane, then n = lane + 64: the accumulation order of k_demod_fm's loop)
        float const t0 = cnrm(va[i]);
        sum_t += t0;
        sum_a += sqrtf(t0);
        float const t1 = cnrm(vb[i]);
        sum_t += t1;
        sum_a += sqrtf(t1);
      }
      sum_t = wave_sum(sum_t);
      sum_a = wave_sum(sum_a);
      FmBlockStats const st = fm_block_stats(sum_t, sum_a, olen);
      int carry = -1, pvc = -1;  // last strong sample and the one before it
#pragma unroll
      for (int h = 0; h < 2; h++) {
        bool const valid = cnrm(h ? vb[i] : va[i]) > st.thr;
        unsigned long long const m = __ballot(valid);
        if (m) {
          int const top = top_bit(m);
          unsigned long long const rest = m & ~(1ull << top);
          pvc = rest ? 64 * h + top_bit(rest) : carry;
          carry = 64 * h + top;
        }
      }
      wave_sync();
      if (lane == 0) fm_record_stats(rec, k, st, carry, pvc, Sk);
    }
    __syncthreads();
    // ---- B: squelch counters and what every block starts from
    if (wave == 0) fm_phase_b(rec, cr, nb);
    __syncthreads();
    // ---- C: discriminator and hold rule (fm.c:116-160), samples from LDS, detected samples into FO[k + 1]
    for (int k = wave; k < nb; k += W) {
      FmBlockReadings const r = fm_block_discriminate<olen>(g, S + k * olen, Y, FO + (k + 1) * olen, olen, fm_threshold(rec.r_amp[k]),
                                                            rec.r_st_in[k], rec.r_la_in[k], rec.r_sq[k]);
      if (lane == 0) {
        rec.r_blanked[k] = r.blanked;
        rec.r_foff[k] = r.foff;
        rec.r_pdev[k] = r.pdev;
      }
    }
    __syncthreads();
    // ---- D (wave 0): carried readings and the status records; the other waves start on the audio filter meanwhile
    if (wave == 0) fm_phase_d(rec, cr, g, pl, c, b0, nb, noise_gain, compute_n0, olen);
    // ---- audio: REAL -> REAL de-emphasis overlap-save on pairs of blocks (fm.c:162-171), FO row k + 1 = block b0 + k
    // (the transform's constants are formed here and not at the top: held across phases A - C they spill)
    Audio256 af;
    if (!flat) af.init(lane, ch.aresp + (size_t)c * 129);
    for (int pr = (wave + W - 1) % W; pr < (nb + 1) / 2; pr += W) {  // (wave 1 takes pair 0: wave 0 is busy with phase D)
      int const k = 2 * pr;
      bool const have1 = k + 1 < nb;
      const float *pm = FO + k * olen, *cm = pm + olen, *nm = cm + olen;
      float const p0 = pm[lane], p1 = pm[lane + 64], c0 = cm[lane], c1 = cm[lane + 64];
      float const n0 = have1 ? nm[lane] : 0.f, n1 = have1 ? nm[lane + 64] : 0.f;
      float *aud0 = pl.audio + ((size_t)c * g.max_blocks + b0 + k) * (2 * (size_t)olen);
      float *aud1 = aud0 + 2 * olen;
      if (flat) {  // fm.c:164-172: no filter, no gain
        aud0[lane] = c0;
        aud0[lane + 64] = c1;
        if (have1) {
          aud1[lane] = n0;
          aud1[lane + 64] = n1;
        }
        continue;
      }
      float2 y2, y3;
      af.run(make_float2(p0, c0), make_float2(p1, c1), make_float2(c0, n0), make_float2(c1, n1), y2, y3);
      aud0[lane] = y2.x * gain;  // fm.c:169-170
      aud0[lane + 64] = y3.x * gain;
      if (have1) {
        aud1[lane] = y2.y * gain;
        aud1[lane + 64] = y3.y * gain;
      }
    }
    __syncthreads();
    // the chunk's last block precedes the next chunk (and, after the last chunk, the next call: filter.c:164)
    if (threadIdx.x < olen) {
      float const v = FO[nb * olen + threadIdx.x];
      FO[threadIdx.x] = v;
      if (b0 + 64 >= nblocks) hist_out[(size_t)c * olen + threadIdx.x] = v;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) cr.store(ch, c);
}

// PL tone tracker (fm.c:236-277): per FM channel, blocks in sequence: append the PL filter output to the
// 16384-sample ring; after every >= 512 new samples transform the ring (in storage order, as the reference
// does) and pick the peak bin.  One workgroup per channel; the ring transform runs in LDS (128 KiB).
__global__ void __launch_bounds__(1024) k_pl_track(Geom g, ChanDev ch, Planes pl, const float2 *__restrict__ tw,
                                                   const int *__restrict__ list, int nblocks) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ float red_e[16];
  __shared__ float red_p[16];
  __shared__ int red_i[16];
  constexpr int FS = 16384;  // (1 << 19) / 32, fm.c:225
  int const c = list[blockIdx.x];
  float *ring = ch.plring + (size_t)c * FS;
  int ptr = ch.pl_ptr[c], last = ch.pl_last[c];
  float plfreq = ch.plfreq[c];
  float const pl_samprate = g.dsamprate / 32.f;
  // The blocks between two transforms are taken together: their PL samples (contiguous in plout) go into the ring in one
  // sweep and their status records in another -- block by block this was a chain of 64 tiny dependent steps per call.
  for (int b = 0; b < nblocks;) {
    int need = (512 - last + g.pl_l - 1) / g.pl_l;  // blocks until fm.c:251's count is reached
    if (need < 1) need = 1;
    int const nb = min(need, nblocks - b);
    const float *src = pl.plout + ((size_t)c * g.max_blocks + b) * g.pl_l;
    for (int i = threadIdx.x; i < nb * g.pl_l; i += blockDim.x) ring[(ptr + i) & (FS - 1)] = src[i];
    ptr = (ptr + nb * g.pl_l) & (FS - 1);
    last += nb * g.pl_l;
    float const before = plfreq;  // what the blocks in front of the one that completes the count report
    if (last >= 512) {  // fm.c:251
      last = 0;
      __syncthreads();
      for (int i = threadIdx.x; i < FS; i += blockDim.x) lds[bitrev((unsigned)i, 14)] = make_float2(ring[i], 0.f);
      lds_fft<-1>(lds, 14, tw, g.tw_log2);
      float tot = 0, pe = 0;
      int pb = -1;
      for (int n = 1 + threadIdx.x; n < FS / 2; n += blockDim.x) {  // skip DC (fm.c:260)
        float const e = cnrm(lds[n]);
        tot += e;
        if (e > pe) {
          pe = e;
          pb = n;
        }
      }
      // block reduction: total energy, and the first bin holding the maximum energy
      tot = wave_sum(tot);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        float const oe = __shfl_xor(pe, o, 64);
        int const ob = __shfl_xor(pb, o, 64);
        if (oe > pe || (oe == pe && ob >= 0 && (pb < 0 || ob < pb))) {
          pe = oe;
          pb = ob;
        }
      }
      int const w = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) {
        red_e[w] = tot;
        red_p[w] = pe;
        red_i[w] = pb;
      }
      __syncthreads();
      tot = 0;
      pe = 0;
      pb = -1;
      for (int k = 0; k < (int)(blockDim.x >> 6); k++) {
        tot += red_e[k];
        if (red_p[k] > pe || (red_p[k] == pe && red_i[k] >= 0 && (pb < 0 || red_i[k] < pb))) {
          pe = red_p[k];
          pb = red_i[k];
        }
      }
      if (pb > 0 && pe > 0.01f * tot) {  // fm.c:271-276
        float const f = (float)pb * pl_samprate / FS;
        if (f > 67 && f < 255) plfreq = f;
      } else {
        plfreq = NAN;
      }
      __syncthreads();
    }
    for (int j = threadIdx.x; j < nb; j += blockDim.x)
      pl.status[(size_t)c * g.max_blocks + b + j].plfreq = j == nb - 1 ? plfreq : before;
    b += nb;
  }
  if (threadIdx.x == 0) {
    ch.pl_ptr[c] = ptr;
    ch.pl_last[c] = last;
    ch.plfreq[c] = plfreq;
  }
}

void launch_pl_track(hipStream_t s, const Geom &g, const ChanDev &ch, const Planes &pl, const float2 *tw, const int *list_fm,
                     int n_fm, int nblocks) {
  if (n_fm <= 0 || g.pl_n <= 0) return;
  ensure_dynamic_lds((const void *)k_pl_track, (size_t)(16384 * 8));
  hipLaunchKernelGGL(k_pl_track, dim3(n_fm), dim3(1024), 16384 * 8, s, g, ch, pl, tw, list_fm, nblocks);
}

// dynamic LDS of the generic FM demodulator: k_demod_fm's samples and discriminator outputs per wave; k_fm_audio's
// audio master, its transform, the PL slave and the twiddles
// waves per channel of k_demod_fm: as many as fit 96 KiB of LDS at 12 bytes a sample, at most 16 or one per block
static int fm_disc_waves(const Geom &g, int nblocks) {
  int const fit = (int)((96u * 1024u) / (12u * (unsigned)g.olen));
  return std::max(1, std::min({16, fit, nblocks}));
}
static size_t fm_disc_lds_bytes(const Geom &g, int waves = 1) { return (size_t)g.olen * 12 * waves; }
static size_t fm_audio_lds_bytes(const Geom &g) {
  return (size_t)g.Ndec * (8 + 4) + (size_t)g.pl_n * 8 + (size_t)(g.dNdec.log2n < 0 ? g.Ndec : g.Ndec / 2) * 8;
}
size_t demod_fm_lds_bytes(const Geom &g) { return std::max(fm_disc_lds_bytes(g), fm_audio_lds_bytes(g)); }

void launch_demod_fm(hipStream_t s, const Geom &g, const ChanDev &ch, const Planes &pl, const float2 *tw, const int *list_fm,
                     int n_fm, int nblocks, int compute_n0, float *fmout, const float *fm_hist_in, float *fm_hist_out) {
  if (n_fm <= 0) return;
  bool const cfg2 = g.Ndec == 256 && g.olen == 128 && g.Mdec == 129;  // cfg 2's geometry
  if (cfg2 && g.pl_n == 0) {  // without the PL measurement: one fused launch
    hipLaunchKernelGGL(k_demod_fm256, dim3(n_fm), dim3(512), 0, s, g, ch, pl, fm_hist_in, fm_hist_out, list_fm, nblocks, compute_n0);
    return;
  }
  int const waves = fm_disc_waves(g, nblocks);
  size_t const lds_a = fm_disc_lds_bytes(g, waves), lds_b = fm_audio_lds_bytes(g);
  ensure_dynamic_lds((const void *)k_demod_fm, lds_a);
  ensure_dynamic_lds((const void *)k_fm_audio, lds_b);
  hipLaunchKernelGGL(k_demod_fm, dim3(n_fm), dim3(64 * waves), lds_a, s, g, ch, pl, fmout, list_fm, nblocks, compute_n0);
  if (cfg2 && g.pl_n == 8 && g.pl_l == 4)  // with the PL measurement: the audio filter and the PL slave in registers
    hipLaunchKernelGGL(k_fm_audio256, dim3(n_fm, (nblocks + 1) / 2), dim3(64), 0, s, g, ch, pl, fmout, fm_hist_in, fm_hist_out,
                       list_fm, nblocks);
  else  // one wave per block up to a 512-point audio master; four from there on (the transform's passes are loops over the
        // workgroup with a barrier each: tools/bench_mixed.py)
    hipLaunchKernelGGL(k_fm_audio, dim3(n_fm, nblocks), dim3(g.Ndec >= 1024 ? 256 : 64), lds_b, s, g, ch, pl, tw, fmout, fm_hist_in,
                       fm_hist_out, list_fm, nblocks);
}

}  // namespace kq
