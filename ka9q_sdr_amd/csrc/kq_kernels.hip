// kq_kernels.hip -- the kernels around the filter and the demodulators: what brings a call's samples and parameters in
// and carries its results out.
//
//   ensure_dynamic_lds      the per-(kernel, device) dynamic-LDS limit every launcher with a large carve goes through
//   k_ingest                int16/int8/float I/Q -> float2 ring, scaled           (radio.c:110-122)
//   k_block_energy_sum      IF power: per-block partial sums of |s|^2 (radio.c:123), and on the workgroups behind them the
//                           call's parameter block, the row-paired samples and the retuned channels' planes
//   k_block_energy_iir      ... and its halving recurrence (radio.c:143-145) as a launch of its own
//   k_ctl_apply             the control-plane records of a call (kq_ctl.hpp)
//   k_copy_to_host          audio and status planes -> pinned host memory
//   k_copy_pcm_to_host      the same as int16 in network byte order, status whole or compact
//   k_pcm                   float -> int16 on the device, with the all-zero chunk mask
//
// The filter kernels: kq_filter_full.hip (generic), kq_full16k.hip, kq_pruned.hip.  The demodulators: kq_demod_fm.hip
// (FM, generic geometry), kq_demod64.hip, kq_pll.hip.  The compat surface's single transforms: kq_single.hip.
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

#include "kq_device.hpp"
#include "kq_ctl.hpp"
#include "kq_energy.hpp"
#include "kq_ldsfft.hpp"

namespace kq {

void ensure_dynamic_lds(const void *kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, size_t> limit;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lock(mu);
  size_t &cur = limit[{kernel, dev}];
  if (bytes > cur) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    cur = bytes;
  }
}

// ---------------------------------------------------------------- ingest
__global__ void k_ingest(const void *__restrict__ src, int format, float2 *__restrict__ dst, size_t n, float gain) {
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float2 v;
    if (format == KQ_IQ_S16) {
      short2 const q = reinterpret_cast<const short2 *>(src)[i];
      float const sc = 1.f / 32767.f;  // SCALE16, radio.c:38
      v = make_float2(q.x * sc, q.y * sc);
    } else if (format == KQ_IQ_S8) {
      char2 const q = reinterpret_cast<const char2 *>(src)[i];
      float const sc = 1.f / 127.f;  // SCALE8, radio.c:39
      v = make_float2(q.x * sc, q.y * sc);
    } else {
      v = reinterpret_cast<const float2 *>(src)[i];
    }
    dst[i] = make_float2(v.x * gain, v.y * gain);  // radio.c:122
  }
}

void launch_ingest(hipStream_t s, const void *src, int format, float2 *dst, size_t nsamples, float gain) {
  if (nsamples == 0) return;
  int const threads = 256;
  size_t blocks = (nsamples + threads - 1) / threads;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_ingest, dim3((unsigned)blocks), dim3(threads), 0, s, src, format, dst, nsamples, gain);
}

// Sum |s|^2 over the L new samples of each block (radio.c:123), `split` workgroups per block (a block alone is 15 trips
// of one workgroup at cfg 4: latency, with 32 of 256 CUs busy), each taking every split-th trip of 1024 samples and
// leaving its partial sum in sums[block * split + part].  The workgroups behind the summing ones carry
// the call's parameter block (oscillator planes + update flags) from the pinned host staging slot into device
// memory, 8 bytes per thread straight over the bus: a hipMemcpyAsync in front of this kernel cost ~25 us of idle
// stream per call (copy-engine start-up), this costs nothing.
// Workgroups 0 .. nblocks*split-1: energy; then the copy of the call's staged parameters; then
// (paired != null) the window's history rows.  `paired`: the samples written out once more with their 512-sample rows
// interleaved in pairs, for k_filter_full16k's 16-byte loads (kq_full16k.hip: out[1024 r + 2 c + e] = in[512 (2 r + e)
// + c]) -- the kernel reads every new sample anyway.  L and hist are multiples of 1024 then.
// `prev` != null, the steady state (no oscillator has been set, no channel has come or gone since the call before): the
// eight oscillator planes are not carried over the bus at all but ADVANCED on the device from the planes of the call
// before -- phase(n + adv) = phase + f adv + r adv (adv - 1) / 2, f + r adv (osc.c:39-51 in closed form, as the host's
// Osc::rebase does it), the history's oscillator = the current one, the shift oscillator advanced by adv_out output
// samples -- and only the per-block flag bytes come from the host.  At 32768 channels the planes are 2 MiB per call and
// took 144 us of the call's 1.6 ms to fetch over the link, 8 bytes per thread.
__device__ __forceinline__ double frac_turns(double ph, double f, double n) {
  // ph + f n modulo one turn: the product split exactly (hi + lo = f n to 106 bits), its whole turns dropped before the sum
  double const hi = f * n, lo = __fma_rn(f, n, -hi);
  double const p = ph + ((hi - floor(hi)) + lo);
  return p - floor(p);
}
__global__ void k_block_energy_sum(const float2 *__restrict__ x, int L, float *__restrict__ sums, int nblocks, int split,
                                   const unsigned long long *__restrict__ params_host,
                                   unsigned long long *__restrict__ params_dev, unsigned nwords, int copy_wgs,
                                   float2 *__restrict__ paired, int hist, const double *__restrict__ prev, unsigned nchan,
                                   unsigned cmax, double adv, double adv_out, int hist_wgs,
                                   const unsigned long long *__restrict__ patch_rec, int npatch,
                                   const unsigned long long *__restrict__ patch_bits) {
  int const pcol = 2 * (threadIdx.x & 511) + (threadIdx.x >> 9);  // place of sample (row parity, column) within its pair of rows
  int const nsum = nblocks * split;
  if ((int)blockIdx.x >= nsum + copy_wgs + hist_wgs) {
    // the channels retuned since the last call (kq_bank.hpp: patch_list): their planes as the host staged them, records of
    // (channel index, eight values) in pinned memory.  The advancing threads below leave exactly these channels alone
    // (patch_bits: one bit per channel, staged with the records), so the two never write the same place.
    int const j = ((int)blockIdx.x - nsum - copy_wgs - hist_wgs) * (int)blockDim.x + (int)threadIdx.x;
    if (j >= npatch) return;
    const unsigned long long *r = patch_rec + (size_t)j * 9;
    unsigned const c = (unsigned)r[0];
    if (c >= cmax) return;
    double *planes = reinterpret_cast<double *>(params_dev);
#pragma unroll
    for (int k = 0; k < 8; k++) planes[(size_t)k * cmax + c] = __longlong_as_double((long long)r[1 + k]);
    return;
  }
  if ((int)blockIdx.x >= nsum + copy_wgs) {  // history: copy only, 8192 samples per workgroup
    int const base = ((int)blockIdx.x - nsum - copy_wgs) * 8192;
    for (int j = 0; j < 8 && base + 1024 * j < hist; j++) paired[base + 1024 * j + pcol] = (x - hist)[base + 1024 * j + threadIdx.x];
    return;
  }
  if ((int)blockIdx.x >= nsum) {
    unsigned const i = (blockIdx.x - nsum) * blockDim.x + threadIdx.x;
    if (!prev) {
      if (i < nwords) params_dev[i] = params_host[i];
      return;
    }
    if (i < nchan) {
      if (patch_bits && ((patch_bits[i >> 6] >> (i & 63)) & 1ull)) return;  // a patched channel: the patch role writes its planes
      double *out = reinterpret_cast<double *>(params_dev);
      double const ph = prev[i], f = prev[cmax + i], r = prev[2 * (size_t)cmax + i];
      double const sp = prev[3 * (size_t)cmax + i], sf = prev[4 * (size_t)cmax + i];
      double p = frac_turns(ph, f, adv);
      if (r != 0.0) {
        p += r * (0.5 * adv * (adv - 1.0));
        p -= floor(p);
      }
      double const f2 = f + r * adv;
      out[i] = p;
      out[cmax + i] = f2;
      out[2 * (size_t)cmax + i] = r;
      out[3 * (size_t)cmax + i] = frac_turns(sp, sf, adv_out);
      out[4 * (size_t)cmax + i] = sf;
      out[5 * (size_t)cmax + i] = p;
      out[6 * (size_t)cmax + i] = f2;
      out[7 * (size_t)cmax + i] = r;
    } else if (i - nchan < nwords - 8 * cmax) {  // the per-block flags behind the planes
      params_dev[8 * (size_t)cmax + (i - nchan)] = params_host[8 * (size_t)cmax + (i - nchan)];
    }
    return;
  }
  __shared__ float red_f[16];
  __shared__ int red_i[16];
  int const blk = (int)blockIdx.x / split, part = (int)blockIdx.x % split;
  const float2 *p = x + (size_t)blk * L;
  float acc = 0;
  int dummy = 0;
  int const first = part * (int)blockDim.x + (int)threadIdx.x, stride = split * (int)blockDim.x;
  // four trips' loads in flight at a time (a workgroup has three or four trips in all: one memory latency, not one each)
  float2 *o = paired ? paired + hist + (size_t)blk * L : nullptr;
  for (int i0 = first; i0 < L; i0 += 4 * stride) {  // blockDim.x = 1024 = one pair of rows per trip
    float2 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = i0 + j * stride < L ? p[i0 + j * stride] : make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int const i = i0 + j * stride;
      if (i < L) {
        acc += cnrm(v[j]);
        if (o) o[(i - (int)threadIdx.x) + pcol] = v[j];
      }
    }
  }
  block_sum_fi(acc, dummy, red_f, red_i);
  if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}
// the IF-power recurrence as a launch of its own (kq_energy.hpp; the full-spectrum filter kernel runs it on the side instead)
__global__ void k_block_energy_iir(const float *__restrict__ sums, int split, const unsigned char *__restrict__ update,
                                   int nblocks, int L, float *__restrict__ state, float *__restrict__ if_power) {
  block_energy_iir_wave(sums, split, update, nblocks, L, state, if_power, (int)threadIdx.x);
}

int block_energy_split(int L) {
  int const trips = (L + 1023) / 1024;
  return std::max(1, std::min(kEnergySplitMax, (trips + 2) / 3));
}

void launch_block_energy_sum(hipStream_t s, const float2 *newsamples, int L, int nblocks, float *sums, const void *params_host,
                             void *params_dev, size_t params_bytes, float2 *paired, int hist, const double *prev_planes,
                             unsigned nchan, unsigned cmax, double adv, double adv_out, const void *patch_records_host, int npatch,
                             const void *patch_bits_host) {
  unsigned const nwords = (unsigned)((params_bytes + 7) / 8);
  // steady state: one thread per channel advances its planes, then the flag words behind the planes are copied
  unsigned const work = prev_planes ? nchan + (nwords - 8 * cmax) : nwords;
  int const copy_wgs = (int)((work + 1023) / 1024);
  int const hist_wgs = paired ? (hist + 8191) / 8192 : 0;
  int const split = block_energy_split(L);
  if (!prev_planes || !patch_records_host || !patch_bits_host) npatch = 0;  // (patches exist in the steady state only)
  int const patch_wgs = (npatch + 1023) / 1024;
  hipLaunchKernelGGL(k_block_energy_sum, dim3(nblocks * split + copy_wgs + hist_wgs + patch_wgs), dim3(1024), 0, s, newsamples, L, sums,
                     nblocks, split, static_cast<const unsigned long long *>(params_host),
                     static_cast<unsigned long long *>(params_dev), nwords, copy_wgs, paired, hist, prev_planes, nchan, cmax, adv,
                     adv_out, hist_wgs, static_cast<const unsigned long long *>(patch_records_host), npatch,
                     npatch ? static_cast<const unsigned long long *>(patch_bits_host) : nullptr);
}

// Control-plane writes (kq_bank.hpp CtlQueue): what kq_bank_set_filter / add_channel / set_mode ... change on the device,
// gathered by the host in pinned memory since the last call and applied here in ONE launch -- as separate small copies each
// cost the stream 10-20 us of switching between kernel and copy packets (a kq_bank_set_filter came to 0.8 ms of pipeline
// time on a bank at real time, tools/soak_realtime.py).  Record r (32 bytes at the front of the buffer): destination, byte
// count (a multiple of 4), then the offset of its payload in the buffer (kind 0), a 32-bit fill value (kind 1) or the
// device address to copy from (kind 2: a value an earlier kernel of the call left on the device -- the noise gain of a
// response designed in front of the filter pass, kq_design.hip design_launch).
__global__ void __launch_bounds__(256) k_ctl_apply(const unsigned char *__restrict__ q) { ctl_apply_record(q, blockIdx.x, threadIdx.x, 256); }
void launch_ctl_apply(hipStream_t s, const void *queue_host, int nrec) {
  if (nrec > 0) hipLaunchKernelGGL(k_ctl_apply, dim3(nrec), dim3(256), 0, s, static_cast<const unsigned char *>(queue_host));
}

void launch_block_energy_iir(hipStream_t s, const float *sums, int L, int nblocks, const unsigned char *update, float *energy_state,
                             float *if_power) {
  hipLaunchKernelGGL(k_block_energy_iir, dim3(1), dim3(64), 0, s, sums, block_energy_split(L), update, nblocks, L, energy_state,
                     if_power);
}

// Device planes -> pinned host memory, 16 bytes per thread and trip, by a handful of workgroups that stay resident
// (kq_bank_pull_planes_async).  hipMemcpyAsync was measured first: with the filter kernel of the next call filling
// every CU the runtime served these device-to-host copies with its own blit kernel, whose workgroups queued behind the
// filter's -- 1.1 ms for 17 MB, and the filter kernel disturbed (rocprofv3 --memory-copy-trace: __amd_rocclr_copyBuffer,
// no SDMA transfer).  These few workgroups are launched the moment the demodulators finish, take their slots before the
// next filter launch fills the rest, and stream at the link's rate (the stores are posted writes over PCIe).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// audio: rows of `row` floats per channel-block of which the first status.nout hold samples (mono: half of a row) -- only
// those travel; 16 lanes take one row, 16 bytes per lane and trip.  status: the whole plane.  rows = channels * max_blocks.
__global__ void __launch_bounds__(256) k_copy_to_host(const float *__restrict__ audio, float *__restrict__ haudio, int row,
                                                      const kq_chan_status *__restrict__ status, u32x4 *__restrict__ hstatus,
                                                      size_t rows, size_t status16) {
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  size_t const tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (haudio) {
    int const sub = (int)(tid & 15);
    for (size_t r = tid >> 4; r < rows; r += stride >> 4) {
      int const n = min(status[r].nout, row);
      const float *src = audio + r * row;
      float *dst = haudio + r * row;
      for (int i = 4 * sub; i < n; i += 64) {  // row and nout are multiples of 4 here (the caller checks), rows 16-byte aligned
        u32x4 const v = *reinterpret_cast<const u32x4 *>(src + i);
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(dst + i));
      }
    }
  }
  const u32x4 *sp = reinterpret_cast<const u32x4 *>(status);
  if (hstatus)
    for (size_t i = tid; i < status16; i += stride) __builtin_nontemporal_store(sp[i], hstatus + i);
}
void launch_copy_to_host(hipStream_t s, const float *audio, float *haudio, int row, const kq_chan_status *status, void *hstatus,
                         size_t rows) {
  // As few workgroups as the transfer needs: one pushes ~4.4 GB/s over the link whatever it has in flight, and every wave
  // of this kernel displaces a workgroup of the filter pass running beside it (with_host_io at cfg 4, 12.6 MB per call:
  // 1.59 ms per step with 32 workgroups, 1.48 with 4-8, 1.64 with 2, which no longer finish inside the step).  One per
  // 2 MiB is 26 GB/s at cfg 4.
  size_t const bytes = rows * ((haudio ? (size_t)row * sizeof(float) : 0) + (hstatus ? sizeof(kq_chan_status) : 0));
  unsigned const wgs = (unsigned)std::min<size_t>(64, std::max<size_t>(4, (bytes + (2u << 20) - 1) >> 21));
  hipLaunchKernelGGL(k_copy_to_host, dim3(wgs), dim3(256), 0, s, audio, haudio, row, status, (u32x4 *)hstatus, rows,
                     rows * sizeof(kq_chan_status) / 16);
}

// The same delivery in the reference's own output format: float -> clipped int16 in network byte order (scaleclip,
// audio.c:22-28; htons at audio.c:48,98 -- the arithmetic of k_pcm below) on the way out, half the bytes over the link.
// 16 lanes take one row, 8 words (two 16-byte loads, one 16-byte store) per lane and trip; 480 = 60 x 8, so a lane's 8
// words never straddle one of the 480-word chunks whose all-zero test decides whether the reference sends the packet
// (audio.c:49,99,105): mask bit k = chunk k of the row is all zero.  The word itself is kq_lane.hpp's pcm_word_be.
// COMPACT: instead of the whole 64-byte status records, the 24 bytes a receiver reads per block (kq_chan_status_compact:
// bb_power, n0, snr, FM foffset / AM + linear agc.gain, FM squelch counter / AM + linear hang counter, nout) -- at real
// time the status plane is half of the PCM delivery's bytes.  A workgroup packs 256 records into LDS and stores them as
// whole 16-byte pieces (6144 bytes per trip, 16-byte aligned whatever the trip).
template <bool COMPACT>
__global__ void __launch_bounds__(256) k_copy_pcm_to_host(const float *__restrict__ audio, short *__restrict__ hpcm,
                                                          unsigned *__restrict__ hmask, int row,
                                                          const kq_chan_status *__restrict__ status, u32x4 *__restrict__ hstatus,
                                                          size_t rows, size_t status16, const int *__restrict__ mode,
                                                          int max_blocks) {
  size_t const stride = (size_t)gridDim.x * blockDim.x;
  size_t const tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int const sub = (int)(tid & 15);
  for (size_t r = tid >> 4; r < rows; r += stride >> 4) {
    int const n = min(status[r].nout, row);
    const float *src = audio + r * row;
    short *dst = hpcm + r * row;
    unsigned nonzero = 0;  // bit k: this lane saw a non-zero word in chunk k
    for (int i = 8 * sub; i < n; i += 128) {  // row and nout are multiples of 8 here (the caller checks)
      float4 const a = *reinterpret_cast<const float4 *>(src + i), c = *reinterpret_cast<const float4 *>(src + i + 4);
      u32x4 v;
      v.x = pcm_word_be(a.x) | (pcm_word_be(a.y) << 16);
      v.y = pcm_word_be(a.z) | (pcm_word_be(a.w) << 16);
      v.z = pcm_word_be(c.x) | (pcm_word_be(c.y) << 16);
      v.w = pcm_word_be(c.z) | (pcm_word_be(c.w) << 16);
      if ((v.x | v.y | v.z | v.w) != 0) nonzero |= 1u << (i / 480);
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(dst + i));
    }
    // (the 16 lanes of a row run the same number of trips +-1 and meet again here: rows are handed out 16 lanes at a time)
    for (int m = 1; m < 16; m <<= 1) nonzero |= __shfl_xor(nonzero, m, 16);
    if (sub == 0 && hmask) {
      int const chunks = (n + 479) / 480;
      hmask[r] = ~nonzero & (chunks >= 32 ? 0xffffffffu : ((1u << chunks) - 1u));
    }
  }
  if (!hstatus) return;
  if constexpr (COMPACT) {
    __shared__ __attribute__((aligned(16))) unsigned rec[256 * 6];
    size_t const trips = (rows + 255) / 256;
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {  // (uniform per workgroup: the barriers are safe)
      size_t const r0 = trip * 256, r = r0 + threadIdx.x;
      if (r < rows) {
        kq_chan_status const st = status[r];
        bool const fm = mode[r / (size_t)max_blocks] == KQ_FM_DEMOD;
        unsigned *o = rec + 6 * threadIdx.x;
        o[0] = __float_as_uint(st.bb_power);
        o[1] = __float_as_uint(st.n0);
        o[2] = __float_as_uint(st.snr);
        o[3] = __float_as_uint(fm ? st.foffset : st.agc_gain);
        o[4] = (unsigned)(fm ? st.squelch_count : st.hangcount);
        o[5] = (unsigned)st.nout;
      }
      __syncthreads();
      size_t const nrec = min((size_t)256, rows - r0);
      unsigned const words = (unsigned)nrec * 6, full = words / 4;
      u32x4 *dst = reinterpret_cast<u32x4 *>(reinterpret_cast<unsigned *>(hstatus) + r0 * 6);  // r0 * 24 bytes: a multiple of 16
      for (unsigned i = threadIdx.x; i < full; i += 256)
        __builtin_nontemporal_store(reinterpret_cast<const u32x4 *>(rec)[i], dst + i);
      if (threadIdx.x < words - 4 * full)  // the last trip's odd record: its trailing 8 bytes
        reinterpret_cast<unsigned *>(dst)[4 * full + threadIdx.x] = rec[4 * full + threadIdx.x];
      __syncthreads();
    }
  } else {
    const u32x4 *sp = reinterpret_cast<const u32x4 *>(status);
    for (size_t i = tid; i < status16; i += stride) __builtin_nontemporal_store(sp[i], hstatus + i);
  }
}
void launch_copy_pcm_to_host(hipStream_t s, const float *audio, short *hpcm, unsigned *hmask, int row,
                             const kq_chan_status *status, void *hstatus, size_t rows, const int *mode_compact, int max_blocks) {
  size_t const sbytes = hstatus ? (mode_compact ? sizeof(kq_chan_status_compact) : sizeof(kq_chan_status)) : 0;
  size_t const bytes = rows * ((size_t)row * sizeof(short) + 4 + sbytes);
  unsigned const wgs = (unsigned)std::min<size_t>(64, std::max<size_t>(4, (bytes + (2u << 20) - 1) >> 21));
  if (mode_compact)
    hipLaunchKernelGGL(k_copy_pcm_to_host<true>, dim3(wgs), dim3(256), 0, s, audio, hpcm, hmask, row, status, (u32x4 *)hstatus, rows,
                       rows * sizeof(kq_chan_status) / 16, mode_compact, max_blocks);
  else
    hipLaunchKernelGGL(k_copy_pcm_to_host<false>, dim3(wgs), dim3(256), 0, s, audio, hpcm, hmask, row, status, (u32x4 *)hstatus, rows,
                       rows * sizeof(kq_chan_status) / 16, mode_compact, max_blocks);
}

// ---------------------------------------------------------------- PCM output stage
// float -> clipped int16 in network byte order (audio.c:22-28, htons at audio.c:48,98) and the all-zero test per
// 480-word chunk that decides whether the reference sends the packet (audio.c:49,99,105).  One wave per channel-block.
__global__ void __launch_bounds__(64) k_pcm(Geom g, Planes pl, short *__restrict__ pcm, unsigned *__restrict__ mask,
                                            const int *__restrict__ chan_list) {
  int const c = chan_list ? chan_list[blockIdx.x] : (int)blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  size_t const cb = (size_t)c * g.max_blocks + b;
  int const nout = pl.status[cb].nout;
  const float *a = pl.audio + cb * 2 * (size_t)g.olen;
  short *o = pcm + cb * 2 * (size_t)g.olen;
  unsigned m = 0;
  int chunk_id = 0;
  for (int base = 0; base < nout; base += 480, chunk_id++) {
    int const len = min(480, nout - base);
    int any = 0;
    for (int i = lane; i < len; i += 64) {
      float const x = a[base + i];
      int v;
      if (x >= 1.0f)
        v = 32767;
      else if (x <= -1.0f)
        v = -32768;
      else
        v = (int)(32767.f * x);  // truncation, as the (short) cast of audio.c:27
      unsigned const h = (unsigned)v & 0xffffu;
      unsigned const be = ((h << 8) | (h >> 8)) & 0xffffu;
      o[base + i] = (short)be;
      any |= (int)be;
    }
    if (__ballot(any != 0) == 0ull) m |= 1u << chunk_id;
  }
  if (lane == 0) mask[cb] = m;
}

void launch_pcm(hipStream_t s, const Geom &g, const Planes &pl, short *pcm, unsigned *mask, int nchan, int nblocks,
                const int *chan_list) {
  hipLaunchKernelGGL(k_pcm, dim3(nchan, nblocks), dim3(64), 0, s, g, pl, pcm, mask, chan_list);
}

}  // namespace kq
