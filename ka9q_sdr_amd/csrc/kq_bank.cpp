// kq_bank.cpp -- host side of the channel bank: the C ABI of include/ka9q_hip.h, in five units (kq_bank.hpp has the map).
//
// Host responsibilities (control plane, once per call or per retune -- never per sample):
//   * NCO bookkeeping in closed form.  The reference advances a complex-double phasor one sample at
//     a time (osc.c:39-51); here each oscillator is (phase, step, sweep) at a reference sample index
//     and the kernels evaluate phase(n) = phase + step*k + sweep*k*(k-1)/2 themselves.
//     In the steady state (nothing set, added or removed since the call before) the device advances every channel's
//     planes itself and the host touches no per-channel state; a retuned channel travels as one 72-byte patch record.
//   * the control plane: set_filter / set_mode / add / remove / set_n0 ... never touch the device.  They gather write
//     records (CtlQueue: filter side, demodulator side) and design jobs (DesignQueue) in pinned memory; the next call
//     applies them with one launch each, in front of its own kernels, behind the calls in flight.  A new filter's
//     response is designed on the bank's stream by kq_design.hip's kernel, straight into the channel's row.
//   * ring management, kernel sequencing, streaming host I/O (copy streams, pinned planes), RTP in and out
//   * one lock per handle (every entry point; let go of while an entry point waits for the device)
//
// This unit owns the error text (g_err), version and device count, pinned host memory for callers, create / destroy,
// sync / join, and the timing figures.
// Lock: kq_bank_create and kq_bank_destroy take none (nobody else has the handle yet / any more); kq_bank_join, _sync,
// _enable_timing and _get_timing take it through BankScope, _get_host_timing and _worst_lock_holder through LockOnly;
// kq_bank_stream, _audio_device_ptr, _status_device_ptr and _fwd_mode take none.  kq_bank_sync lets go of it (Unlocked) while
// it waits for the streams.  ensure_events, report_lost_sibling, sync_all, drain_timing want it held by the caller.
#include <cstdarg>

#include "kq_bank.hpp"

using namespace kq::bank;

namespace {
thread_local std::string g_err;

int ilog2(unsigned v) {
  int l = 0;
  while ((1u << l) < v) l++;
  return l;
}
}  // namespace

// the text kq_last_error() returns: every translation unit of the library reports through this (kq_host.hpp)
void kq_internal_set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

namespace kq::bank {

int ensure_events(kq_bank *b, std::vector<EventPair> &v, size_t need) {
  while (v.size() < need) {
    EventPair p;
    if (b->new_event(&p.a, hipEventDefault) || b->new_event(&p.b, hipEventDefault)) return -1;
    v.push_back(p);
  }
  return 0;
}

// the N = 65536 kernel's "a sibling never showed up" flag (pinned host memory): reported once, by whichever of
// kq_bank_sync / kq_bank_host_io_wait the host uses to wait -- a streaming host never calls the former
int report_lost_sibling(kq_bank *b) {
  if (b->big.err && *b->big.err) {
    *b->big.err = 0;
    kq_internal_set_error("N = 65536 filter: a sibling workgroup's compute_n0 sum never arrived (n0 of that call is NaN)");
    return -1;
  }
  return 0;
}

int sync_all(kq_bank *b) {
  KQ_TRY(hipStreamSynchronize(b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream2));
  // the streaming copies too: "everything issued so far" (kq_bank_sync) includes a plane copy still in flight
  if (b->copy_in) KQ_TRY(hipStreamSynchronize(b->copy_in));
  if (b->copy_out) KQ_TRY(hipStreamSynchronize(b->copy_out));
  return 0;
}

int drain_timing(kq_bank *b) {
  if (sync_all(b)) return -1;
  for (int k = 0; k < kq_bank::kSlots; k++) harvest_slot(b, k);
  std::vector<EventPair> *sets[3] = {&b->ev_filter, &b->ev_demod, &b->ev_ingest};
  double *dst[3] = {&b->acc.filter_ms, &b->acc.demod_ms, &b->acc.ingest_ms};
  for (int k = 0; k < 3; k++) {
    for (size_t i = 0; i < b->ev_used[k]; i++) {
      float ms = 0;
      KQ_TRY(hipEventElapsedTime(&ms, (*sets[k])[i].a, (*sets[k])[i].b));
      *dst[k] += ms;
    }
    b->ev_used[k] = 0;
  }
  return 0;
}

}  // namespace kq::bank

extern "C" {

const char *kq_last_error(void) { return g_err.c_str(); }
const char *kq_version(void) { return "ka9q_hip 0.1 (gfx950)"; }
int kq_abi_version(void) { return KQ_ABI_VERSION; }

int kq_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

void *kq_host_alloc(size_t bytes) {
  void *p = nullptr;
  hipError_t const e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
  if (e != hipSuccess) {
    kq_internal_set_error("hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}
void kq_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

namespace {
// kq_bank_create in three steps: what can be refused from the configuration alone ...
static int create_check(const kq_bank_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("NULL config");
    return -1;
  }
  unsigned const N = cfg->L + cfg->M - 1;
  // FFTW plans any N (filter.c:78); here a power of two, or -- on the generic kernels, one LDS block -- an even 2^a 3^b 5^c 7^d
  // up to 16384 (a front end whose rate is not 48 kHz x 2^k: 240 kHz gives decimate 5, radio_status.c:266)
  bool const n_pow2 = (N & (N - 1)) == 0;
  if (cfg->L == 0 || cfg->M < 2 || N < 16 || (!n_pow2 && (!kq::fft_size_ok((int)N) || N > 65536))) {
    kq_internal_set_error("L+M-1 = %u must be a power of two >= 16, or an even 2^a 3^b 5^c 7^d in 16..65536", N);
    return -1;
  }
  if (cfg->decimate < 1 || N % cfg->decimate != 0 || cfg->L % cfg->decimate != 0 || (cfg->M - 1) % cfg->decimate != 0) {
    kq_internal_set_error("decimate %u must be >= 1 and divide N, L and M-1", cfg->decimate);
    return -1;
  }
  // decimate = samprate / 48000 = 1 (radio_status.c:266: a 48 kHz front end, a sound-card receiver): the slave's transform is
  // as long as the master's and needs a buffer of its own beside it in LDS (k_filter_full)
  if (cfg->decimate == 1 && N > 8192) {
    kq_internal_set_error("decimate 1 needs L+M-1 = %u <= 8192 (master and slave transform side by side in LDS)", N);
    return -1;
  }
  unsigned const Ndec = N / cfg->decimate;
  if (Ndec < 4 || ((Ndec & (Ndec - 1)) != 0 && (!kq::fft_size_ok((int)Ndec) || Ndec > 16384))) {
    kq_internal_set_error("N/decimate = %u must be a power of two >= 4, or an even 2^a 3^b 5^c 7^d in 4..16384", Ndec);
    return -1;
  }
  if (cfg->max_channels == 0 || cfg->max_blocks == 0 || cfg->samprate <= 0) {
    kq_internal_set_error("max_channels, max_blocks and samprate must be positive");
    return -1;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    kq_internal_set_error("no HIP device available (the gfx950 kernels are the only compute path)");
    return -1;
  }
  if (cfg->device < 0 || cfg->device >= ndev) {
    kq_internal_set_error("device %d out of range (%d visible)", cfg->device, ndev);
    return -1;
  }
  return 0;
}

// ... the geometry and the forward path that follow from it ...
static int create_geometry(kq_bank *b) {
  const kq_bank_config *cfg = &b->cfg;
  unsigned const N = cfg->L + cfg->M - 1, Ndec = N / cfg->decimate;
  kq::Geom &g = b->g;
  g.N = (int)N;
  g.L = (int)cfg->L;
  g.M = (int)cfg->M;
  g.D = (int)cfg->decimate;
  g.Ndec = (int)Ndec;
  g.olen = (int)(cfg->L / cfg->decimate);           // filter.c:116
  g.Mdec = (int)((cfg->M - 1) / cfg->decimate + 1); // filter.c:514
  g.log2N = ilog2(N);
  g.log2Ndec = ilog2(Ndec);
  g.samprate = cfg->samprate;
  g.tw_log2 = g.log2N < 16 ? 16 : g.log2N;  // the PL tracker (16384) and the PLL carrier search (65536) need these periods
  {
    // pltask geometry (fm.c:201-205): decimate 32 from the audio master; needs a usable transform size
    int const pn = g.Ndec / 32, plen = g.olen / 32;
    // (where 32 does not divide N/decimate or the block, create_filter_output warns and truncates both, filter.c:103-107,116:
    //  the slave then resamples by N_dec / PL_N instead of 32 and the tone reads that much off -- what the reference does, and
    //  what happens here; only a PL_N this library has no transform for -- odd, or with a prime factor beyond 7 -- has no PL slave)
    bool const ok = pn >= 4 && plen >= 1 && !cfg->pl_tone_off && ((pn & (pn - 1)) == 0 || kq::fft_size_ok(pn));
    g.pl_n = ok ? pn : 0;
    g.pl_l = ok ? plen : 0;
  }
  {  // the generic path's transform plans (powers of two: no tables)
    bool ok_n = false, ok_d = false, ok_p = true;
    g.dN = kq::fft_dim(g.N, &ok_n);
    g.dNdec = kq::fft_dim(g.Ndec, &ok_d);
    g.dPl = g.pl_n > 0 ? kq::fft_dim(g.pl_n, &ok_p) : kq::FftDim{};
    if (!ok_n || !ok_d || !ok_p) {
      kq_internal_set_error("transform plan for N = %d / N/decimate = %d failed", g.N, g.Ndec);
      return -1;
    }
  }
  g.max_blocks = (int)cfg->max_blocks;
  g.dsamprate = (float)cfg->samprate / cfg->decimate;

  // N = 65536 with compute_n0 (cfg 5 as the reference runs it), or the full path asked for by name: the 16384-point
  // register kernel in four sibling workgroups per channel-block
  bool const can64k = kq::full64k_supported(g);
  bool const can_prune = kq::pruned_supported(g) && !cfg->compute_n0;
  if (cfg->fwd_mode == KQ_FWD_PRUNED) {
    if (!can_prune) {
      kq_internal_set_error("pruned forward path unavailable for this geometry or with compute_n0 enabled");
      return -1;
    }
    b->fwd_mode = KQ_FWD_PRUNED;
  } else if (cfg->fwd_mode == KQ_FWD_FULL) {
    b->fwd_mode = KQ_FWD_FULL;
  } else {
    // N/D = 256 (cfg 2): the pruned kernel is correct but slower than the full-spectrum kernel (2.24 vs 0.45 ms per
    // 16384 channel-blocks), so AUTO keeps the full path there; KQ_FWD_PRUNED still selects it explicitly
    b->fwd_mode = (can_prune && g.Ndec != 256) ? KQ_FWD_PRUNED : KQ_FWD_FULL;
  }
  b->use64k = b->fwd_mode == KQ_FWD_FULL && can64k;
  if (b->fwd_mode == KQ_FWD_FULL && N > 16384 && !b->use64k && (!kq::split_supported(g) || cfg->compute_n0)) {
    kq_internal_set_error("N = %u: the full path beyond 16384 points needs N = 65536, or compute_n0 off and a split N = S x N1 with N1 <= 16384 a "
                          "size of its own (N = 32768; 19200, 24000, 38400, 48000 ...) and N/D small enough to sit beside it in LDS", N);
    return -1;
  }
  return 0;
}

// ... and everything the handle owns from the start.  The buffers are cleared on the main stream, which is waited for once,
// behind the last of them: no stream ever sees one uncleared
static int create_alloc(kq_bank *b) {
  const kq_bank_config *cfg = &b->cfg;
  kq::Geom const &g = b->g;
  if (b->open_stream(cfg->stream)) return -1;
  size_t const C = cfg->max_channels, B = cfg->max_blocks;
  // max_blocks blocks plus L - 1 samples of slack: a partly filled block never stands in the way of a batch that fits the
  // ring as such (kq_bank_push_rtp); kq_bank_process still takes at most max_blocks blocks per call
  b->ring_cap = (size_t)(g.M - 1) + B * (size_t)g.L + (size_t)(g.L - 1);
  if (b->alloc(&b->ring[0], b->ring_cap, true)) return -1;
  if (b->alloc(&b->ring[1], b->ring_cap, true)) return -1;
  if (!(b->tw = kq::half_twiddles(g.tw_log2))) {
    kq_internal_set_error("kq_bank_create: no twiddle table of period 2^%d", g.tw_log2);
    return -1;
  }
  if (b->alloc(&b->chd.mode, C, true)) return -1;
  if (b->alloc(&b->chd.flags, C, true)) return -1;
  if (b->alloc(&b->chd.low, C, true)) return -1;
  if (b->alloc(&b->chd.high, C, true)) return -1;
  if (b->alloc(&b->chd.resp, C * g.Ndec, true)) return -1;
  if (b->alloc(&b->chd.aresp, C * (g.Ndec / 2 + 1), true)) return -1;
  if (b->alloc(&b->chd.fm_gain, C, true)) return -1;
  if (b->alloc(&b->chd.headroom, C, true)) return -1;
  if (b->alloc(&b->chd.recovery, C, true)) return -1;
  if (b->alloc(&b->chd.hangmax, C, true)) return -1;
  if (b->alloc(&b->chd.noise_gain, C, true)) return -1;
  if (b->alloc(&b->chd.hist_len, C, true)) return -1;
  if (b->alloc(&b->chd.hist2_len, C * kq::kOldLevels, true)) return -1;
  if (b->alloc(&b->chd.hist2_osc, 3 * C * kq::kOldLevels, true)) return -1;
  // compute_n0's lane masks (build_n0mask), where a register-resident kernel reads them: N = 65536 has four sub-transforms' worth
  if (b->cfg.compute_n0 && (kq::full16k_supported(g) || b->use64k)) {
    size_t const nsub = b->use64k ? 4 : 1;
    if (b->alloc(&b->chd.n0lane, C * nsub * 256, true)) return -1;
    if (b->alloc(&b->chd.n0meta, C * nsub, true)) return -1;
    if (b->alloc(&b->chd.n0slot, C, true)) return -1;
  }
  if (b->use64k) {
    if (b->alloc(&b->big.sync, C * cfg->max_blocks * 12, true)) return -1;
    if (b->alloc(&b->big.n0part, C * cfg->max_blocks * 4, true)) return -1;
    if (b->alloc(&b->big.xs, C * cfg->max_blocks * (size_t)g.Ndec, true)) return -1;
    if (b->alloc_pinned(&b->big.err, 1)) return -1;
    *b->big.err = 0;
  }
  // eight oscillator planes | the per-block IF-power flags | the list of channels retuned since the last call
  for (int k = 0; k < 2; k++)
    if (b->alloc(&b->osc_dev2[k], 8 * C + (B + sizeof(double) - 1) / sizeof(double) + (C * sizeof(int) + 7) / 8, true)) return -1;
  // (chd's oscillator planes -- lo_*, sh_*, hist_phase / _freq / _rate -- are set per call, to the call's parity)
  // the demodulators' own stream (run_blocks says when it is used); KQ_DEMOD_OVERLAP=0 leaves it out
  const char *ov = getenv("KQ_DEMOD_OVERLAP");
  b->overlap_mode = ov ? (atoi(ov) != 0 ? 1 : 0) : -1;
  bool const overlap = b->overlap_mode != 0;
  if (!overlap) b->stream2 = b->stream;
  // (its stream at high priority -- so that the demodulators' few workgroups are placed ahead of the next filter launch's --
  // was measured in round 4: with_host_io 0.50 -> 0.78-1.25 ms at cfg 2, 1.45 -> 1.72 at cfg 4; at the LOWEST priority --
  // so that the next call's first kernels are not dispatched behind the demodulators' waiting workgroups -- round 5:
  // 1.483 -> 1.692 ms per call at 32768 channels x 2 blocks, the demodulators starve until the filter pass ends and the
  // call after next waits for them; default priority it is)
  if (overlap && b->new_stream(&b->stream2)) return -1;
  for (hipEvent_t &e : b->ev_demod_done)
    if (b->new_event(&e, hipEventDisableTiming)) return -1;
  b->stage_bytes = 8 * C * sizeof(double) + ((B + 7) & ~(size_t)7) + ((C * sizeof(int) + 7) & ~(size_t)7);  // copied in 8-byte words
  b->patch_off = b->stage_bytes;               // the retune patches' records (never copied as a whole: the patch role of k_block_energy_sum reads them)
  b->stage_bytes += (size_t)kq_bank::kMaxPatch * kq_bank::kPatchBytes;
  b->bits_off = b->stage_bytes;
  b->stage_bytes += ((C + 63) / 64) * sizeof(unsigned long long);
  static_assert(kq_bank::kSlots == 4, "slot_bit_words");
  for (int k = 0; k < kq_bank::kSlots; k++) {
    if (b->alloc_pinned(&b->stage_host[k], b->stage_bytes) || b->new_event(&b->stage_ev[k], hipEventDefault) ||
        b->new_event(&b->stage_t0[k], hipEventDefault))
      return -1;
    memset(b->stage_host[k] + b->bits_off, 0, b->stage_bytes - b->bits_off);
  }
  if (b->alloc(&b->chd.fm_state, C, true)) return -1;
  if (b->alloc(&b->chd.lastaudio, C, true)) return -1;
  if (b->alloc(&b->chd.sq_count, C, true)) return -1;
  if (b->alloc(&b->chd.ahist, C * (size_t)(g.Mdec > 1 ? g.Mdec - 1 : 1), true)) return -1;
  if (!kq::demod64_supported(g)) {
    if (b->alloc(&b->fmout, C * B * (size_t)g.olen, true)) return -1;
    for (float *&h : b->fm_hist)
      if (b->alloc(&h, C * (size_t)(g.Mdec > 1 ? g.Mdec - 1 : 1), true)) return -1;
  }
  if (b->alloc(&b->chd.foffset, C, true)) return -1;
  if (b->alloc(&b->chd.pdev, C, true)) return -1;
  if (b->alloc(&b->chd.gain, C, true)) return -1;
  if (b->alloc(&b->chd.hang, C, true)) return -1;
  if (b->alloc(&b->chd.dc, C, true)) return -1;
  if (b->alloc(&b->chd.n0, C, true)) return -1;
  if (b->alloc(&b->chd.pl_ptr, C, true)) return -1;
  if (b->alloc(&b->chd.pl_last, C, true)) return -1;
  if (b->alloc(&b->chd.plfreq, C, true)) return -1;
  if (g.pl_n > 0) {
    if (b->alloc(&b->chd.plresp, (size_t)g.pl_n / 2 + 1, true)) return -1;
    if (b->alloc(&b->chd.plring, C * 16384, true)) return -1;
  }
  if (b->alloc(&b->pl.audio, C * B * 2 * (size_t)g.olen, true)) return -1;
  if (b->alloc(&b->pl.status, C * B, true)) return -1;
  for (int k = 0; k < 2; k++) {  // filter -> demod hand-over planes, one set per call parity
    b->pl2[k].audio = b->pl.audio;
    b->pl2[k].status = b->pl.status;
    if (b->alloc(&b->pl2[k].filt, C * B * g.olen, true)) return -1;
    if (b->alloc(&b->pl2[k].n0raw, C * B, true)) return -1;
    if (b->alloc(&b->pl2[k].if_power, B * (1 + kq::kEnergySplitMax), true)) return -1;  // + the partial sums of k_block_energy_sum
    if (g.pl_n > 0 && b->alloc(&b->pl2[k].plout, C * B * g.pl_l, true)) return -1;
  }
  b->pl = b->pl2[0];
  if (b->alloc(&b->energy_state, 2, true)) return -1;
  if (kq::full16k_paired_supported(g) && b->alloc(&b->win_paired, (size_t)(g.M - 1) + (size_t)B * g.L, true)) return -1;
  for (int *&l : b->list_dev)
    if (b->alloc(&l, C, true)) return -1;
  for (kq_bank::CtlQueue &q : b->ctl)
    for (int k = 0; k < kq_bank::CtlQueue::kDepth; k++)
      if (b->alloc_pinned(&q.buf[k], kq_bank::CtlQueue::kBytes) || b->new_event(&q.applied[k], hipEventDisableTiming)) return -1;
  {
    kq_bank::DesignQueue &d = b->dq;
    size_t const per_job = (size_t)g.Ndec * sizeof(float2);
    d.max_jobs = (unsigned)std::max<size_t>(1, std::min<size_t>(kq_bank::DesignQueue::kMax, ((size_t)64 << 20) / per_job));
    if (b->alloc(&d.scratch, (size_t)d.max_jobs * g.Ndec, true)) return -1;
    if (b->alloc(&d.ng_next, 2 * C, true)) return -1;
    for (int k = 0; k < kq_bank::DesignQueue::kDepth; k++)
      if (b->alloc_pinned(&d.pin[k], kq_bank::DesignQueue::kMax * (sizeof(kq::DesignJob) + sizeof(kq::DesignTarget))) ||
          b->new_event(&d.read[k], hipEventDisableTiming))
        return -1;
    for (hipEvent_t &e : d.ng_moved)
      if (b->new_event(&e, hipEventDisableTiming)) return -1;
    if (g.Ndec <= 16384 && kq::design_prepare(g.olen, g.Mdec)) return -1;  // (the twiddle table of the design kernel, built now)
  }
  if (b->alloc(&b->list_active_dev, C, true)) return -1;
  if (b->alloc(&b->list_active_ds_dev, C, true)) return -1;
  if (b->alloc(&b->chd.fflags, C, true)) return -1;
  if (b->alloc(&b->list_unswept_dev, C, true)) return -1;
  if (b->alloc(&b->list_swept_dev, C, true)) return -1;
  if (b->fwd_mode == KQ_FWD_PRUNED && b->alloc(&b->chan_tw, C * kq::pruned_table_elems(g), true)) return -1;
  if (b->fwd_mode != KQ_FWD_PRUNED && kq::full16k_supported(g) && b->alloc(&b->chd.row_ph, C * 32, true)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));  // the clears are over: the blocking copies below do not meet them
  if (g.pl_n > 0) {
    // PL low-pass: bins with 0 < f < 300 Hz, Kaiser beta 2.0 (fm.c:207-218)
    int const PL_M = g.pl_n - g.pl_l + 1;
    std::vector<kq::cfloat> r(g.pl_n / 2 + 1, kq::cfloat(0, 0));
    for (int j = 0; j <= g.pl_n / 2; j++) {
      float const f = (float)j * g.dsamprate / g.Ndec;
      if (f > 0 && f < 300) r[j] = 1;
    }
    if (kq::window_rfilter(g.pl_l, PL_M, r, 2.0)) return -1;
    KQ_TRY(hipMemcpy(b->chd.plresp, r.data(), r.size() * sizeof(float2), hipMemcpyHostToDevice));
  }
  {
    std::vector<float> nanv(C, NAN);
    KQ_TRY(hipMemcpy(b->chd.plfreq, nanv.data(), C * sizeof(float), hipMemcpyHostToDevice));
  }
  return 0;
}
}  // namespace

kq_bank *kq_bank_create(const kq_bank_config *cfg) {
  if (create_check(cfg)) return nullptr;
  // the handle lives on cfg->device; the calling thread's current device is put back on the way out, error paths
  // included, like every other entry point (kq_device.hpp DeviceScope)
  kq::DeviceScope dev_scope_(cfg->device);
  {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) {
      kq_internal_set_error("hipSetDevice(%d) failed", cfg->device);
      return nullptr;
    }
  }
  kq_bank *b = new kq_bank();
  b->cfg = *cfg;
  b->chans.reserve(cfg->max_channels);  // the elements never move (kq_bank_rtp_from_planes keeps an address past the lock)
  if (create_geometry(b) || create_alloc(b)) {
    kq_bank_destroy(b);
    return nullptr;
  }
  return b;
}

int kq_bank_destroy(kq_bank *b) {
  kq::DeviceScope dev_scope_(b ? b->cfg.device : -1);  // (not the handle's lock: nobody else may be using a handle that is being destroyed)
  if (!b) return 0;
  b->close();
  delete b;
  return 0;
}

void *kq_bank_stream(kq_bank *b) { return b ? (void *)b->stream : nullptr; }

int kq_bank_join(kq_bank *b) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  if (b->calls == 0) return 0;
  int const last = (int)((b->calls - 1) & 1);
  if (b->demod_overlapped[last]) KQ_TRY(hipStreamWaitEvent(b->stream, b->ev_demod_done[last], 0));
  return 0;
}

int kq_bank_sync(kq_bank *b) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  // "everything issued so far" includes what the control plane has queued for the next call: applied now
  if (ctl_flush_now(b)) return -1;
  hipStream_t const st[4] = {b->stream, b->stream2, b->copy_in, b->copy_out};  // (read under the lock)
  {
    Unlocked u(dev_scope_);
    for (hipStream_t x : st)
      if (x) KQ_TRY(hipStreamSynchronize(x));
  }
  return report_lost_sibling(b);
}

void *kq_bank_audio_device_ptr(kq_bank *b) { return b ? b->pl.audio : nullptr; }
void *kq_bank_status_device_ptr(kq_bank *b) { return b ? b->pl.status : nullptr; }

int kq_bank_enable_timing(kq_bank *b, int on) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  if (!on && b->timing) drain_timing(b);
  b->timing = on;  // 0 off, 1 filter kernel only, >= 2 every scope
  return 0;
}

int kq_bank_get_timing(kq_bank *b, kq_timing *t, int reset) {
  BankScope dev_scope_(b);
  if (!b || !t) return -1;
  if (drain_timing(b)) return -1;
  *t = b->acc;
  if (reset) b->acc = kq_timing{};
  return 0;
}

int kq_bank_get_host_timing(kq_bank *b, kq_host_timing *t, int reset) {
  if (!b || !t) return -1;
  LockOnly lk(b);
  *t = b->host_acc;
  if (reset) {
    b->host_acc = kq_host_timing{};
    b->worst_holder = "";
  }
  return 0;
}

const char *kq_bank_worst_lock_holder(kq_bank *b) {
  if (!b) return "";
  LockOnly lk(b);
  return b->worst_holder;  // (a function name: static storage)
}

int kq_bank_fwd_mode(const kq_bank *b) { return b ? b->fwd_mode : -1; }

}  // extern "C"
