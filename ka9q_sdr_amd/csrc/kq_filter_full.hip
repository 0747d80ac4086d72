// kq_filter_full.hip -- the pre-detection filter for any geometry, one workgroup per (channel, block) with the whole
// transform in LDS (the fast paths for particular sizes: kq_full16k.hip, kq_pruned.hip).
//
//   k_filter_full       NCO mix -> N-point FFT in LDS -> [compute_n0] -> response multiply / CROSS_CONJ -> N/D-point IFFT
//                       -> last olen samples      (radio.c:132-139, filter.c:151, radio.c:383-425, filter.c:206-250)
//   k_filter_split      the same for N beyond one LDS block: N = S * N1, only the N/D bins the slave reads are combined
//   split_factor / split_supported: which N the split form takes
#include "kq_device.hpp"
#include "kq_ldsfft.hpp"

namespace kq {

// ---------------------------------------------------------------- full-FFT pre-detection filter
// grid (channel, block); dynamic LDS = N float2.
__global__ void k_filter_full(Geom g, ChanDev ch, Planes pl, const float2 *__restrict__ window,
                              const float2 *__restrict__ tw, int compute_n0, float2 *__restrict__ spec_dump, int spec_ch,
                              const int *__restrict__ chan_list) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ float red_f[16];
  __shared__ int red_i[16];
  int const c = chan_list ? chan_list[blockIdx.x] : (int)blockIdx.x, b = blockIdx.y;
  int const N = g.N, Ndec = g.Ndec;

  // --- NCO mix (radio.c:132-139): closed form of the phasor recurrence of osc.c:39-51
  double const ph0 = ch.lo_phase[c], f0 = ch.lo_freq[c], r = ch.lo_rate[c];
  double const hp0 = ch.hist_phase[c], hf0 = ch.hist_freq[c], hr = ch.hist_rate[c];
  const float2 *x = window + (size_t)b * g.L;
  double const mbase = (double)b * g.L;
  // One oscillator over the whole window and no sweep (every block but the first one after a retune, every channel that is
  // not Doppler-tracked): a thread's samples are blockDim apart, so its phasor advances by one constant step; evaluated afresh
  // in double every fourth sample, three float products in between (3 x 6e-8 of rounding against the 1e-5 of the parity bar).
  // The per-sample evaluation in double was 800 of this kernel's 1 770 vector instructions per wave (tools/pmc_sq.sh).
  // (samples of an old oscillator: the first hist_len[c] of the call's first window, ChanDev -- block b's window has those
  //  that lie beyond its start, if the history planes differ from the current ones at all)
  bool const same_osc = hr == r && hp0 == ph0 && hf0 == f0;
  int const n_old = same_osc ? 0 : ch.hist_len[c] - b * g.L;
  // (... and of the oscillators before that one, where a channel was retuned again inside M - 1 samples: hist2_*)
  OlderOsc older;
  load_older(ch, c, b * g.L, n_old > 0, older);
  bool const one_osc = r == 0.0 && n_old <= 0;
  if (one_osc) {
    float2 const step = phasor_turns(f0 * (double)blockDim.x);
    float2 lo = make_float2(1.f, 0.f);
    int k = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x, k++) {
      lo = (k & 3) ? cmul(lo, step) : phasor_turns(ph0 + f0 * (mbase + i));
      lds[fft_pos((unsigned)i, g.dN)] = cmul(x[i], lo);
    }
  } else {
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      double const m = mbase + i;
      bool const old = i < n_old;  // mixed before the retune took effect: pre-retune oscillator(s)
      double pp = old ? hp0 : ph0, ff = old ? hf0 : f0, rr = old ? hr : r;
      pick_older(older, i, pp, ff, rr);
      double turns = pp + ff * m;
      if (rr != 0.0) turns += rr * (0.5 * m * (m - 1.0));
      float2 const lo = phasor_turns(turns);
      lds[fft_pos((unsigned)i, g.dN)] = cmul(x[i], lo);
    }
  }
  fft_any<-1>(lds, g.dN, tw, g.tw_log2);  // filter.c:151

  if (spec_dump != nullptr && c == spec_ch) {
    float2 *o = spec_dump + (size_t)b * N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) o[i] = lds[i];
  }

  // --- compute_n0 (radio.c:383-425), status only
  if (compute_n0) {
    float const low = ch.low[c], high = ch.high[c];
    float avg = INFINITY;
    for (int iter = 0; iter < 2; iter++) {
      float acc = 0;
      int bins = 0;
      for (int n = threadIdx.x; n < N; n += blockDim.x) {
        int const k = (n <= N / 2) ? n : n - N;
        // the reference forms k*samprate in int (radio.c:407,409): keep its 32-bit wrap
        int const prod = (int)((unsigned)k * (unsigned)g.samprate);
        float const f = (float)prod / N;
        if (f >= low && f <= high) continue;
        float const p = cnrm(lds[n]);
        if (p < avg * 2) {
          acc += p;
          bins++;
        }
      }
      block_sum_fi(acc, bins, red_f, red_i);
      avg = acc / bins;
    }
    if (threadIdx.x == 0) pl.n0raw[(size_t)c * g.max_blocks + b] = (float)(avg / (2.0 * N * g.samprate));
  }

  // --- slave: response multiply (filter.c:206-227), CROSS_CONJ (filter.c:239-249)
  // G goes to the unused middle of the spectrum buffer: bins N_dec/2+1 .. N-N_dec/2 are never read
  // (decimate 1: there is no such middle -- every bin is read -- and the launch has asked for a second buffer behind the first)
  float2 *G = Ndec == N ? lds + N : lds + (Ndec / 2 + 1);
  const float2 *H = ch.resp + (size_t)c * Ndec;
  bool const isb = (ch.fflags[c] & FLAG_ISB) != 0;
  for (int p = threadIdx.x; p <= Ndec / 2; p += blockDim.x) {
    float2 gp = cmul(H[p], lds[p]);
    if (p > 0 && p < Ndec / 2) {
      int const k = Ndec - p;
      float2 gn = cmul(H[k], lds[N - p]);
      if (isb) {
        float2 const pos = gp, neg = gn;
        gp = cadd(pos, cconj(neg));
        gn = csub(neg, cconj(pos));
      }
      G[fft_pos((unsigned)k, g.dNdec)] = gn;
    }
    G[fft_pos((unsigned)p, g.dNdec)] = gp;
  }
  fft_any<+1>(G, g.dNdec, tw, g.tw_log2);  // filter.c:250

  float2 *o = pl.filt + ((size_t)c * g.max_blocks + b) * g.olen;
  for (int i = threadIdx.x; i < g.olen; i += blockDim.x) o[i] = G[Ndec - g.olen + i];  // filter.c:131
}

void launch_filter_full(hipStream_t s, const Geom &g, const ChanDev &ch, const Planes &pl, const float2 *window,
                        const float2 *tw, int nchan, int nblocks, int compute_n0, float2 *spec_dump, int spec_ch,
                        const int *chan_list) {
  size_t const lds_bytes = (size_t)g.N * sizeof(float2) * (g.Ndec == g.N ? 2 : 1);
  ensure_dynamic_lds((const void *)k_filter_full, lds_bytes);
  // By how many workgroups a CU's 160 KiB of LDS hold: 256 threads where there are four or more of them, 512 where two or
  // three, 1024 where one workgroup has the CU to itself (tools/bench_mixed.py and a sweep over N, filter kernel ms for
  // 1024 channels x 8 blocks at 1024 / 512 / 256 threads: N = 2048 0.33 / 0.16 / 0.13, 4096 0.53 / 0.29 / 0.28,
  // 6144 0.94 / 0.51 / 0.66, 8192 0.90 / 0.64 / 0.74, 9600 1.20 / 0.87 / 1.32, 10240 1.37 / 1.64 / 2.61, 15360 1.74 / 2.10 / 3.44;
  // until round 6 it was 1024 from N = 4096 on)
  int const threads = lds_bytes <= 40 * 1024 ? 256 : 2 * lds_bytes + 512 <= 160 * 1024 ? 512 : 1024;
  hipLaunchKernelGGL(k_filter_full, dim3(nchan, nblocks), dim3(threads), lds_bytes, s, g, ch, pl, window, tw, compute_n0,
                     spec_dump, spec_ch, chan_list);
}

// ---------------------------------------------------------------- full path for N beyond one LDS block
// N = S * N1 with N1 * 8 B <= 128 KiB.  Decimation in time over s: F_s = FFT_N1{ xm[S m + s] } and
// X[k] = sum_s W_N^{s k} F_s[k mod N1]; only the N/D bins the slave reads (filter.c:206-227) are combined,
// into a small side buffer.  Same mix, response multiply, CROSS_CONJ and inverse transform as k_filter_full.
// compute_n0 needs every bin of the N-point spectrum and is not available on this path.
// Round 6: N1 and N/D may carry factors 3 and 5 (d1 / g.dNdec; twN = the full-circle table of N points then), so that a
// bank takes N = 19200, 24000, 38400, 48000 ... as well as 32768.
// grid (channel, block); dynamic LDS = (N1 + N_dec) float2.
__global__ void k_filter_split(Geom g, ChanDev ch, Planes pl, const float2 *__restrict__ window,
                               const float2 *__restrict__ tw, int S, FftDim d1, const float2 *__restrict__ twN,
                               const int *__restrict__ chan_list) {
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int const c = chan_list ? chan_list[blockIdx.x] : (int)blockIdx.x, b = blockIdx.y;
  int const N = g.N, Ndec = g.Ndec, N1 = d1.n;
  float2 *side = lds + N1;  // X at signed bin k, stored at index k mod N_dec
  for (int i = threadIdx.x; i < Ndec; i += blockDim.x) side[i] = make_float2(0.f, 0.f);

  double const ph0 = ch.lo_phase[c], f0 = ch.lo_freq[c], r = ch.lo_rate[c];
  double const hp0 = ch.hist_phase[c], hf0 = ch.hist_freq[c], hr = ch.hist_rate[c];
  const float2 *x = window + (size_t)b * g.L;
  double const mbase = (double)b * g.L;
  int const n_old = (hr == r && hp0 == ph0 && hf0 == f0) ? 0 : ch.hist_len[c] - b * g.L;  // as in k_filter_full
  OlderOsc older;
  load_older(ch, c, b * g.L, n_old > 0, older);
  for (int s = 0; s < S; s++) {
    __syncthreads();
    for (int i = threadIdx.x; i < N1; i += blockDim.x) {
      int const n = S * i + s;
      double const m = mbase + n;
      bool const old = n < n_old;
      double pp = old ? hp0 : ph0, ff = old ? hf0 : f0, rr = old ? hr : r;
      pick_older(older, n, pp, ff, rr);
      double turns = pp + ff * m;
      if (rr != 0.0) turns += rr * (0.5 * m * (m - 1.0));
      lds[fft_pos((unsigned)i, d1)] = cmul(x[n], phasor_turns(turns));
    }
    fft_any<-1>(lds, d1, tw, g.tw_log2);
    for (int q = threadIdx.x; q < Ndec; q += blockDim.x) {
      int const k = (q <= Ndec / 2) ? q : q - Ndec;            // signed bin
      int const src = (k >= 0) ? k : N1 + k;                   // k mod N1
      int idx = (int)(((long long)s * k) % N);                 // W_N^{s k}
      if (idx < 0) idx += N;
      float2 w;
      if (twN) {
        w = twN[idx];
      } else {
        w = tw[(size_t)(idx & (N / 2 - 1)) << (g.tw_log2 - g.log2N)];
        if (idx >= N / 2) w = make_float2(-w.x, -w.y);
      }
      side[q] = cadd(side[q], cmul(w, lds[src]));
    }
  }
  __syncthreads();
  const float2 *H = ch.resp + (size_t)c * Ndec;
  bool const isb = (ch.fflags[c] & FLAG_ISB) != 0;
  float2 *G = lds;
  for (int p = threadIdx.x; p <= Ndec / 2; p += blockDim.x) {
    float2 gp = cmul(H[p], side[p]);
    if (p > 0 && p < Ndec / 2) {
      int const k = Ndec - p;
      float2 gn = cmul(H[k], side[k]);
      if (isb) {
        float2 const pos = gp, neg = gn;
        gp = cadd(pos, cconj(neg));
        gn = csub(neg, cconj(pos));
      }
      G[fft_pos((unsigned)k, g.dNdec)] = gn;
    }
    G[fft_pos((unsigned)p, g.dNdec)] = gp;
  }
  fft_any<+1>(G, g.dNdec, tw, g.tw_log2);
  float2 *o = pl.filt + ((size_t)c * g.max_blocks + b) * g.olen;
  for (int i = threadIdx.x; i < g.olen; i += blockDim.x) o[i] = G[Ndec - g.olen + i];
}

// the split N = S * N1: the smallest S whose N1 is a size the LDS transform takes (a power of two: S = N / 16384)
static int split_factor(const Geom &g) {
  if (g.dN.log2n >= 0) return g.N > 16384 ? g.N >> 14 : 0;
  for (int S = 2; S <= 64; S++)
    if (g.N % S == 0 && g.N / S <= 16384 && fft_size_ok(g.N / S)) return S;
  return 0;
}
bool split_supported(const Geom &g) {
  int const S = g.N > 16384 && g.N <= 65536 ? split_factor(g) : 0;
  return S > 0 && (size_t)g.Ndec * 8 + (size_t)(g.N / S) * 8 <= 160 * 1024 - 256 && g.Ndec <= g.N / S;
}

void launch_filter_split(hipStream_t s, const Geom &g, const ChanDev &ch, const Planes &pl, const float2 *window,
                         const float2 *tw, int nchan, int nblocks, const int *chan_list) {
  int const S = split_factor(g);
  if (S <= 0) return;
  bool ok = false;
  FftDim const d1 = fft_dim(g.N / S, &ok);  // (cached since the bank was created)
  if (!ok) return;
  size_t const lds_bytes = ((size_t)d1.n + g.Ndec) * sizeof(float2);
  ensure_dynamic_lds((const void *)k_filter_split, lds_bytes);
  hipLaunchKernelGGL(k_filter_split, dim3(nchan, nblocks), dim3(1024), lds_bytes, s, g, ch, pl, window, tw, S, d1,
                     g.dN.log2n >= 0 ? (const float2 *)nullptr : g.dN.twc, chan_list);
}

}  // namespace kq
