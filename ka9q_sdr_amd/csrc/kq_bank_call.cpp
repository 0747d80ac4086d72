// kq_bank_call.cpp -- one call: the per-call parameters (eval_planes, stage_call_params), run_blocks and its six steps,
// the retune / patch bookkeeping the steps read (note_retune, note_patch), the filter interval of a staging slot
// (harvest_slot), and the entry points kq_bank_process / _process_resident / _process_spectrum / _blocks_ready.
// Everything a steady-state call executes on the host is in this unit.
// Lock: the three process entry points take it as the receiver (BankScope(b, true): their wait for it is what
// kq_host_timing reports) and let go of it once, in slot_prewait, while they wait for the staging slot's last reader;
// kq_bank_blocks_ready takes it through LockOnly.  Everything else wants it held by the caller.
#include "kq_bank.hpp"

using namespace kq::bank;

namespace kq::bank {

// the filter interval of the call that last used the slot (its closing marker has completed)
void harvest_slot(kq_bank *b, int slot) {
  if (!b->stage_timed[slot]) return;
  b->stage_timed[slot] = false;
  float ms = 0;
  // (a call that failed between the two records leaves an interval that does not exist: dropped, not an error of this call)
  if (hipEventElapsedTime(&ms, b->stage_t0[slot], b->stage_ev[slot]) == hipSuccess && ms > 0) {
    b->acc.filter_ms += ms;
    if (ms > b->acc.filter_max_ms) {
      b->acc.filter_max_ms = ms;
      b->acc.filter_max_submit_ms = b->stage_submit_ms[slot];
      b->acc.filter_max_launch = b->stage_launch[slot];
    }
  } else
    (void)hipGetLastError();
}

// The second LO or the Doppler oscillator of channel `ch` is about to be set: the samples mixed so far keep what they were
// mixed with (radio.c:132-139 mixes sample by sample, osc.c:22-36 changes only what follows), and the next M - 1 of them are
// the history of the windows to come.  Several settings between two calls are one transition (nothing was mixed with the
// ones in between).  A setting while an EARLIER transition is still inside the history -- possible only where M - 1 > L: a
// channel retuned before every block at the reference's default -L 3840 -M 4353 -- moves that one, and any before it, one
// level down the list the kernels know per window (hist2_*: kOldLevels of them beyond the last); one more than that inside
// the same M - 1 samples (M - 1 > 5 L and a retune before every block) drops the oldest.
void note_retune(kq_bank *b, int ch) {
  HostChan &h = b->chans[ch];
  int64_t const hist = (int64_t)b->g.M - 1;
  if (h.retuned && h.hist_old == hist) return;  // set again before anything was mixed with the setting in between
  if (h.retuned) {  // the transition before this one still has samples in the history: it and its elders move one level down
    for (int l = kq::kOldLevels - 1; l > 0; l--) {
      h.lo2_oldx[l] = h.lo2_oldx[l - 1];
      h.dop_oldx[l] = h.dop_oldx[l - 1];
      h.hist_oldx[l] = h.hist_oldx[l - 1];
    }
    h.lo2_oldx[0] = h.lo2_old;
    h.dop_oldx[0] = h.dop_old;
    h.hist_oldx[0] = h.hist_old;
  }
  h.lo2_old = h.lo2;
  h.dop_old = h.dop;
  h.retuned = true;
  h.hist_old = hist;
}

// an oscillator of channel `ch` has been set (or the channel is new): the next call patches its planes -- or, with too
// many of them, stages the whole bank
void note_patch(kq_bank *b, int ch) {
  HostChan &h = b->chans[ch];
  if (h.patched) return;
  if ((int)b->patch_list.size() >= kq_bank::kMaxPatch) {
    b->osc_dirty = true;
    return;
  }
  h.patched = true;
  b->patch_list.push_back(ch);
}

}  // namespace kq::bank

namespace {

// the input mix at sample n as {phase, step, sweep}: the second LO, plus the Doppler NCO while its frequency is non-zero
// (radio.c:135)
void eval_mix(const Osc &lo2, const Osc &dop, int64_t n, double out[3]) {
  double p = lo2.phase_at(n), f = lo2.step_at(n), r = lo2.sweep();
  if (dop.set_f != 0) {
    p += dop.phase_at(n);
    f += dop.step_at(n);
    r += dop.sweep();
  }
  out[0] = p - std::floor(p);
  out[1] = f;
  out[2] = r;
}

// the eight plane values of one channel for a call whose first window starts at absolute sample n_w:
// out = {phase, step, sweep, shift phase, shift step, history phase, history step, history sweep}
void eval_planes(const kq_bank *b, const HostChan &h, int64_t n_w, double out[8]) {
  eval_mix(h.lo2, h.dop, n_w, out);
  double const q = h.shift.phase_at(b->out_abs);
  out[3] = q - std::floor(q);
  out[4] = h.shift.step_at(b->out_abs);
  if (h.retuned)  // history of the first block keeps the pre-retune oscillators
    eval_mix(h.lo2_old, h.dop_old, n_w, out + 5);
  else
    std::copy(out, out + 3, out + 5);
}

// What one call has been asked for and what it has decided so far: the steps of run_blocks_timed fill it in their order and
// read what the steps before them left
struct Call {
  const float2 *window;
  unsigned nblocks;
  const unsigned char *update_host;
  const float2 *spectrum;
  int C;                       // channel slots, holes included
  size_t Cmax;
  bool steady = false;         // the device advances the planes itself (decide_sweeps)
  bool swept_pruned = false;   // pruned forward path with a swept channel
  int pp = 0;                  // the call's parity: which hand-over planes, which oscillator planes
  int64_t n_w = 0;             // absolute index of the first window's first sample
  kq::Planes pl;               // this parity's planes ...
  kq::ChanDev chd;             // ... and the channel tables with this parity's oscillator planes
  int slot = 0, nret = 0, npatch = 0;  // the staging slot; the channels retuned / patched that travel in it
  unsigned nredo = 1;          // leading blocks the retuned channels leave to the per-sample variant
  size_t ret_off = 0;          // of the retune list inside the slot and inside the oscillator planes
  const int *retune_list = nullptr;
  bool use16k = false, plain = false, mixed = false, swept_steady = false, swept64k = false;  // choose_filter_variant
  float2 *paired = nullptr;    // the row-paired copy of the samples, where the steady-state variants read it
  bool iir_off = false, iir_done = false;  // KQ_IIR_IN_FILTER=0; the IF-power recurrence has ridden in a filter launch
};

// Per-call parameters: oscillator phase/step/sweep for a call whose first window starts at absolute
// sample n_w, the shift oscillator at the first output sample, and the IF-power update flags.
// Filled into the next pinned staging slot (k.slot); the first kernel of the call copies it to the device.
// k.steady: the planes are advanced on the device from the call before; only the flags, the retune list (k.nret channels)
// and the patch records of the channels on b->patch_list travel (k.npatch of them).
int stage_call_params(kq_bank *b, Call &k) {
  size_t const C = b->chans.size(), Cmax = b->cfg.max_channels;
  int const slot = k.slot = b->stage_next;
  b->stage_next = (slot + 1) % kq_bank::kSlots;
  auto const tw0 = std::chrono::steady_clock::now();
  KQ_TRY(hipEventSynchronize(b->stage_ev[slot]));  // the call that last read this slot has got past its filter
  auto const tw1 = std::chrono::steady_clock::now();
  b->host_acc.slot_wait_ms += std::chrono::duration<double, std::milli>(tw1 - tw0).count();
  harvest_slot(b, slot);
  double *pl = reinterpret_cast<double *>(b->stage_host[slot]);
  unsigned char *flags = b->stage_host[slot] + 8 * Cmax * sizeof(double);
  memcpy(flags, k.update_host, k.nblocks);
  // the per-block flags sit right behind the eight oscillator planes, in the staging slot and on the device; behind
  // them the channels retuned since the last call (their first block is redone on the per-sample path)
  int *ret = reinterpret_cast<int *>(flags + ((b->cfg.max_blocks + 7) & ~7u));
  b->ret_host.clear();
  {  // the bitmap of the slot's last use goes back to zero
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(b->stage_host[slot] + b->bits_off);
    for (unsigned w : b->slot_bit_words[slot]) bits[w] = 0;
    b->slot_bit_words[slot].clear();
  }
  if (k.steady) {
    unsigned char *rec = b->stage_host[slot] + b->patch_off;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(b->stage_host[slot] + b->bits_off);
    for (int c : b->patch_list) {
      if ((size_t)c >= b->chans.size()) continue;  // (removed since, and dropped from the end)
      HostChan const &h = b->chans[c];
      if (!h.active) continue;
      long long const idx = c;
      memcpy(rec, &idx, sizeof idx);
      double v[8];
      eval_planes(b, h, k.n_w, v);
      memcpy(rec + 8, v, sizeof v);
      rec += kq_bank::kPatchBytes;
      k.npatch++;
      bits[c >> 6] |= 1ull << (c & 63);
      b->slot_bit_words[slot].push_back((unsigned)(c >> 6));
      if (h.retuned) {
        ret[k.nret++] = c;
        b->ret_host.push_back(c);
      }
    }
  } else {
    for (size_t c = 0; c < C; c++) {
      double v[8];
      eval_planes(b, b->chans[c], k.n_w, v);
      for (int i = 0; i < 8; i++) pl[(size_t)i * Cmax + c] = v[i];
    }
    for (size_t c = 0; c < C; c++)
      if (b->chans[c].active && b->chans[c].retuned) {
        ret[k.nret++] = (int)c;
        b->ret_host.push_back((int)c);
      }
  }
  b->host_acc.stage_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count();
  return 0;
}

// a launch over every active channel: all `C` slots, or -- remove_channel has left holes, which are skipped -- the list of
// the active ones (`list_dev`: the copy of it that the launch's stream reads)
struct ChanList {
  int n;
  const int *list;
};
ChanList active_channels(const kq_bank *b, const int *list_dev) {
  bool const holes = b->list_active_host.size() != b->chans.size();
  return holes ? ChanList{(int)b->list_active_host.size(), list_dev} : ChanList{(int)b->chans.size(), nullptr};
}

double sweep_of(HostChan const &h) { return h.lo2.sweep() + (h.dop.set_f != 0 ? h.dop.sweep() : 0.0); }
// the pruned forward path's limits on a swept oscillator
bool sweep_ok(const kq_bank *b, double r) {
  kq::Geom const &g = b->g;
  if (b->fwd_mode != KQ_FWD_PRUNED || r == 0) return true;
  // The pruned kernels take the sweep's cross term r*R*a*b to first order and drop its b^2 part:
  // both must stay far below the 1e-5 parity budget over one window.
  double const cross = 2 * M_PI * std::fabs(r) * (double)g.N * g.D, quad = std::fabs(r) * (double)g.D * g.D * 0.5;
  if (g.Ndec == 256) {
    kq_internal_set_error("swept NCO at N/D = 256 is only available on the full forward path: use KQ_FWD_FULL");
    return false;
  }
  if (cross > 3e-4 || quad > 2e-7) {
    kq_internal_set_error("sweep rate too large for the pruned forward path (cross term %.3g rad): use KQ_FWD_FULL", cross);
    return false;
  }
  return true;
}

// Step 1.  Steady or not, and the launch decisions that depend on the channels' sweeps: counted over all channels when the
// bank is staged afresh, kept up to date from the patch list otherwise.
int decide_sweeps(kq_bank *b, Call &k) {
  kq::Geom const &g = b->g;
  // Per-channel decisions are taken afresh only when something about the channels or their oscillators has changed since
  // the call before (osc_dirty); a steady call walks no per-channel state on the host.
  const char *const steady_env = getenv("KQ_STEADY");  // A/B switch, read per call: 0 = stage every call on the host
  bool const steady_off = steady_env && atoi(steady_env) == 0;
  k.steady = !b->osc_dirty && !k.spectrum && b->calls > 0 && !steady_off;
  if (!k.steady) {
    bool any = false;
    for (HostChan const &h : b->chans) any = any || h.active;
    b->cache_any = any;
  }  // (steady: kept up to date by kq_bank_add_channel / kq_bank_remove_channel)
  if (!b->cache_any) {
    kq_internal_set_error("no channels in bank");
    return -1;
  }
  if (b->lists_dirty && upload_lists(b)) return -1;
  double const fast_limit = sweep_limit(b);
  if (!k.steady) {
    int n_swept = 0, n_fast = 0, n_active = 0;
    for (HostChan &h : b->chans) {
      if (!h.active) continue;
      double const r = sweep_of(h);
      if (!sweep_ok(b, r)) return -1;
      h.r_eff = r;
      n_active++;
      n_swept += r != 0;
      n_fast += std::fabs(r) > fast_limit;
    }
    b->n_swept = n_swept;
    b->n_fast = n_fast;
    b->n_active = n_active;
    b->sweep_lists_dirty = true;
  } else {
    // Rolling re-reference.  The device advances the oscillator planes from call to call; the host's closed forms, which a
    // retune is patched from, are referred to the sample they were last staged at and lose digits as that recedes (f k at
    // k = 2^24: 1e-9 turns).  Until round 5 the whole bank was therefore staged afresh every 2^24 samples -- at 32768
    // channels a call with 0.4-3 ms more host time and 2 MB over the link every 1.68 s: the periodic stall of a paced
    // receiver (tools/rt_stall_diag.sh: long delivery intervals at multiples of 1.68 s).  Now every call moves a few
    // channels' reference up and re-stages just those through the patch records (33 of 32768 per 2-block call), so that
    // each channel comes round at least once per 2^24 samples and no call is different from the others.
    {
      size_t const Cn = b->chans.size();
      double const span = (double)k.nblocks * (double)g.L;
      size_t want = (size_t)((double)Cn * span / (double)(1 << 24)) + 1;
      want = std::min({want, Cn, (size_t)kq_bank::kMaxPatch / 2});
      for (size_t i = 0; i < want && (int)b->patch_list.size() < kq_bank::kMaxPatch / 2; i++) {
        size_t const c = b->refresh_next < Cn ? b->refresh_next : 0;
        b->refresh_next = c + 1;
        HostChan &h = b->chans[c];
        if (!h.active || h.patched) continue;  // (a channel the operator has just set is staged from fresh forms anyway)
        h.lo2.rebase(b->n_abs);
        h.dop.rebase(b->n_abs);
        h.shift.rebase(b->out_abs);
        note_patch(b, (int)c);
      }
    }
    for (int c : b->patch_list) {
      if ((size_t)c >= b->chans.size()) continue;
      HostChan &h = b->chans[c];
      if (!h.active) continue;
      double const r = sweep_of(h);
      if (!sweep_ok(b, r)) return -1;
      if ((r != 0) != (h.r_eff != 0)) b->sweep_lists_dirty = true;
      b->n_swept += (r != 0) - (h.r_eff != 0);
      b->n_fast += (std::fabs(r) > fast_limit) - (std::fabs(h.r_eff) > fast_limit);
      h.r_eff = r;
    }
  }
  k.swept_pruned = b->fwd_mode == KQ_FWD_PRUNED && b->n_swept > 0;
  if (k.swept_pruned) b->chan_tw_dirty = true;  // the step changes from call to call
  return 0;
}

// Step 2.  This parity's planes, the call's parameters into a staging slot, and the history records of the channels whose
// windows still hold samples of an old oscillator.
int stage_history(kq_bank *b, Call &k) {
  kq::Geom const &g = b->g;
  size_t const Cmax = k.Cmax;
  k.pp = (int)(b->calls & 1);
  k.pl = b->pl2[k.pp];
  k.chd = b->chd;
  k.chd.lo_phase = b->osc_dev2[k.pp];
  k.chd.lo_freq = k.chd.lo_phase + Cmax;
  k.chd.lo_rate = k.chd.lo_phase + 2 * Cmax;
  k.chd.sh_phase = k.chd.lo_phase + 3 * Cmax;
  k.chd.sh_freq = k.chd.lo_phase + 4 * Cmax;
  k.chd.hist_phase = k.chd.lo_phase + 5 * Cmax;
  k.chd.hist_freq = k.chd.lo_phase + 6 * Cmax;
  k.chd.hist_rate = k.chd.lo_phase + 7 * Cmax;
  // this parity's hand-over planes were last read by the demodulators two calls ago
  // (asked of the host first: a wait on another stream's event costs the stream a barrier packet, several microseconds
  // of idle device even when the event fired long ago -- and two calls later it always has)
  if (b->demod_overlapped[k.pp] && hipEventQuery(b->ev_demod_done[k.pp]) != hipSuccess)
    KQ_TRY(hipStreamWaitEvent(b->stream, b->ev_demod_done[k.pp], 0));
  k.n_w = b->n_abs - (g.M - 1);
  if (stage_call_params(b, k)) return -1;
  // how far into the call's windows those channels' old samples reach (ChanDev::hist_len; M - 1 right after the retune), and
  // how many leading blocks the kernels that mix a whole window with one oscillator therefore leave to the per-sample variant
  int64_t deepest = 0;
  for (int c : b->ret_host) {
    HostChan &h = b->chans[c];
    deepest = std::max(deepest, h.hist_old);
    int const len = (int)std::min<int64_t>(h.hist_old, INT32_MAX);
    if (h.hist_dev != len) {
      if (ctl_put(b, CTL_FILTER, b->chd.hist_len + c, &len, sizeof len)) return -1;
      h.hist_dev = len;
    }
    for (int l = 0; l < kq::kOldLevels; l++) {
      size_t const i = (size_t)c * kq::kOldLevels + l;
      int const lenx = (int)std::min<int64_t>(h.hist_oldx[l], INT32_MAX);
      if (lenx > 0) {  // (its phase is the window start's: written for every call it lasts)
        double v[3];
        eval_mix(h.lo2_oldx[l], h.dop_oldx[l], k.n_w, v);  // (an older transition, note_retune: as the history planes)
        if (ctl_put(b, CTL_FILTER, b->chd.hist2_osc + 3 * i, v, sizeof v)) return -1;
      }
      if (h.histx_dev[l] != lenx) {
        if (ctl_put(b, CTL_FILTER, b->chd.hist2_len + i, &lenx, sizeof lenx)) return -1;
        h.histx_dev[l] = lenx;
      }
    }
  }
  k.nredo = (unsigned)std::min<int64_t>(k.nblocks, std::max<int64_t>(1, (deepest + g.L - 1) / g.L));
  k.ret_off = 8 * Cmax * sizeof(double) + ((b->cfg.max_blocks + 7) & ~7u);
  k.retune_list = reinterpret_cast<const int *>(reinterpret_cast<const unsigned char *>(b->osc_dev2[k.pp]) + k.ret_off);
  return 0;
}

// Step 3.  Which variant of the filter kernel the call's channels get.
int choose_filter_variant(kq_bank *b, Call &k) {
  // full-spectrum path: the register-resident N = 16384 kernel where it applies
  k.use16k = kq::full16k_supported(b->g);
  // the N = 16384 kernel on the full path, fed with samples: where swept and unswept channels have variants of their own
  bool const sweep_variants = k.use16k && !b->use64k && b->fwd_mode != KQ_FWD_PRUNED && !k.spectrum;
  // No sweep anywhere: the register-resident kernel runs without its per-sample oscillator path; the first block of
  // a channel retuned since the last call (history still on the old oscillator) is then redone below with the
  // general variant, as the pruned path does.
  // (N = 65536: the steady-state variant takes sweeps up to full64k_sweep_limit() itself)
  // (N = 16384: swept channels inside full16k_sweep_limit() have a steady-state variant of their own, `swept_steady`)
  k.plain = b->use64k ? b->n_fast == 0 : b->n_swept == 0;
  k.swept_steady = sweep_variants && b->n_swept > 0 && b->n_fast == 0;
  k.swept64k = b->use64k && b->n_swept > 0;
  // N = 16384 with swept and unswept channels side by side: two launches over two lists (see list_unswept_dev)
  k.mixed = sweep_variants && b->n_swept > 0 && b->n_swept < b->n_active;
  if (k.mixed && b->sweep_lists_dirty) {
    b->list_unswept_host.clear();
    b->list_swept_host.clear();
    for (size_t c = 0; c < b->chans.size(); c++)
      if (b->chans[c].active) (b->chans[c].r_eff != 0 ? b->list_swept_host : b->list_unswept_host).push_back((int)c);
    if (ctl_put(b, CTL_FILTER, b->list_unswept_dev, b->list_unswept_host.data(), b->list_unswept_host.size() * sizeof(int))) return -1;
    if (ctl_put(b, CTL_FILTER, b->list_swept_dev, b->list_swept_host.data(), b->list_swept_host.size() * sizeof(int))) return -1;
    b->sweep_lists_dirty = false;
  }
  // That steady-state variant loads its samples 16 bytes at a time from a copy of the call's samples whose 512-sample
  // rows are interleaved in pairs; the IF-power kernel, which reads every new sample anyway, writes it
  k.paired = ((k.use16k || b->use64k) && (k.plain || k.mixed || k.swept_steady) && b->win_paired && b->fwd_mode != KQ_FWD_PRUNED) ? b->win_paired : nullptr;
  return 0;
}

// before a launch of k_filter_full16k: hand it the IF-power recurrence, once per call
void iir_arm(kq_bank *b, Call &k) {
  b->big.iir = kq::IirArgs{};
  if (k.iir_done || k.iir_off || k.spectrum) return;
  b->big.iir.sums = k.pl.if_power + b->cfg.max_blocks;
  b->big.iir.update = reinterpret_cast<const unsigned char *>(b->osc_dev2[k.pp] + 8 * k.Cmax);
  b->big.iir.state = b->energy_state;
  b->big.iir.if_power = k.pl.if_power;
  b->big.iir.split = kq::block_energy_split(b->g.L);
  b->big.iir.nblocks = (int)k.nblocks;
  b->big.iir.L = b->g.L;
  k.iir_done = true;
}

// One launch of the full-spectrum filter (N <= 16384) over `nch` channels (`list`: which; null: the first nch) and `nbl` blocks.
// variant 0: the general one (what a list of channels retuned since the last call needs); 1: steady state -- the host
// vouches that no channel of THIS launch sweeps; 2: steady state, every one does.  !outputs: no compute_n0, no spectrum dump
void full_launch(kq_bank *b, Call &k, int nch, int nbl, const int *list, int variant, bool outputs = true) {
  int const n0 = outputs ? b->cfg.compute_n0 : 0, dump_ch = outputs ? b->spec_ch : -1;
  float2 *const dump = outputs ? b->spec_dump : nullptr;
  if (k.use16k && b->fwd_mode != KQ_FWD_PRUNED) iir_arm(b, k);  // (not the pruned path's redo launches: they come second)
  if (k.use16k)
    kq::launch_filter_full16k(b->stream, b->g, k.chd, k.pl, k.window, b->tw, nch, nbl, n0, dump, dump_ch, list, variant,
                              variant ? k.paired : nullptr, b->big);
  else
    kq::launch_filter_full(b->stream, b->g, k.chd, k.pl, k.window, b->tw, nch, nbl, n0, dump, dump_ch, list);
}

// one launch of the N = 65536 kernel (four sibling workgroups per channel-block)
void launch64k(kq_bank *b, Call &k, int nch, int nbl, const int *list, bool steady) {
  iir_arm(b, k);
  kq::Big64 big = b->big;
  big.epoch = ++b->big.epoch;  // never 0: the words start out zeroed
  if (big.epoch == 0) big.epoch = ++b->big.epoch;
  kq::launch_filter_full64k(b->stream, b->g, k.chd, k.pl, k.window, b->tw, nch, nbl, b->cfg.compute_n0, b->spec_dump, b->spec_ch,
                            list, steady, k.swept64k, steady ? k.paired : nullptr, big);
}

// the call's filter launches, one of five families: a spectrum handed in, the pruned forward path, N = 65536, a split N
// beyond 16384, the full-spectrum kernels up to 16384
void launch_filter(kq_bank *b, Call &k) {
  kq::Geom const &g = b->g;
  int const nblocks = (int)k.nblocks;
  ChanList const act = active_channels(b, b->list_active_dev);
  if (k.spectrum) {
    // execute_filter_output (filter.c:206-250) and compute_n0 (radio.c:383-425) on the spectrum handed in: one small
    // launch each per channel-block (this is the one-channel, one-block path of the demodulator thread entry points)
    for (int c = 0; c < k.C; c++) {
      if (!b->chans[c].active) continue;
      bool const isb = b->chans[c].cfg.demod_type == KQ_LINEAR_DEMOD && b->chans[c].cfg.isb;
      for (unsigned i = 0; i < k.nblocks; i++) {
        const float2 *X = k.spectrum + (size_t)i * g.N;
        size_t const cb = (size_t)c * g.max_blocks + i;
        if (b->cfg.compute_n0)
          kq::launch_n0_single(b->stream, X, g.N, g.samprate, b->chans[c].cfg.low, b->chans[c].cfg.high, k.pl.n0raw + cb);
        kq::launch_slave_bank(b->stream, X, k.chd.resp + (size_t)c * g.Ndec, k.pl.filt + cb * g.olen, g.N, g.Ndec, g.olen, isb ? 2 : 1,
                              b->tw, g.tw_log2);
      }
    }
  } else if (b->fwd_mode == KQ_FWD_PRUNED) {
    if (b->chan_tw_dirty) {  // the tables depend only on each channel's LO step: rebuild after a retune
      kq::launch_pruned_tables(b->stream, g, k.chd, b->chan_tw, k.C);
      b->chan_tw_dirty = false;
    }
    if (kq::pruned_carries_iir(g)) iir_arm(b, k);
    kq::launch_filter_pruned(b->stream, g, k.chd, k.pl, k.window, b->chan_tw, act.n, nblocks, k.swept_pruned, act.list, b->big.iir);
    b->big.iir = kq::IirArgs{};
    // The pruned kernels assume one oscillator over the whole window.  For the first block after a retune the
    // history half still carries the old one: redo just those channel-blocks on the per-sample path.
    if (k.nret > 0) {
      if (g.N > 16384)
        kq::launch_filter_split(b->stream, g, k.chd, k.pl, k.window, b->tw, k.nret, (int)k.nredo, k.retune_list);
      else
        full_launch(b, k, k.nret, (int)k.nredo, k.retune_list, 0, false);
    }
  } else if (b->use64k) {
    launch64k(b, k, act.n, nblocks, act.list, k.plain);
    // the steady-state variant mixes a whole window with one oscillator: the first block of a channel retuned since
    // the last call (history still on the old one) is redone with the per-sample variant
    if (k.plain && k.nret > 0) launch64k(b, k, k.nret, (int)k.nredo, k.retune_list, false);
  } else if (g.N > 16384) {
    kq::launch_filter_split(b->stream, g, k.chd, k.pl, k.window, b->tw, k.C, nblocks, nullptr);
  } else {
    int const steady_variant = k.swept_steady ? 2 : k.plain ? 1 : 0;  // (of a launch whose channels all sweep, or none)
    // The unswept steady-state variant of the N = 16384 kernel takes its row phasors from chd.row_ph, which depends on the
    // channels' frequency steps only: rebuilt, from the planes this call's launches read, after a step has changed
    // (row_ph_dirty) and whenever the planes were staged afresh.  (A swept channel's row is never read: its step moves
    // from call to call, and the setter that ends the sweep marks the plane.)
    if (k.use16k && (k.plain || k.mixed) && (b->row_ph_dirty || !k.steady)) {
      kq::launch_full16k_rows(b->stream, k.chd, k.C);
      b->row_ph_dirty = false;
    }
    if (k.mixed) {
      full_launch(b, k, (int)b->list_unswept_host.size(), nblocks, b->list_unswept_dev, 1);
      full_launch(b, k, (int)b->list_swept_host.size(), nblocks, b->list_swept_dev, steady_variant);
    } else {  // (nobody sweeps, or everybody does)
      full_launch(b, k, act.n, nblocks, act.list, steady_variant);
    }
    if (k.use16k && (k.plain || k.mixed || k.swept_steady) && k.nret > 0)
      full_launch(b, k, k.nret, (int)k.nredo, k.retune_list, 0);
  }
}

// Step 4.  The control plane's filter-side writes, the IF-power sums (whose launch carries the call's parameters to the
// device), the filter, and the marker behind it.
int launch_energy_and_filter(kq_bank *b, Call &k) {
  kq::Geom const &g = b->g;
  int const slot = k.slot, pp = k.pp;
  // the control plane's filter-side writes since the last call, in front of this call's first kernel
  if (ctl_flush(b, CTL_FILTER, b->stream)) return -1;
  {
    Scope t(b, 2, b->stream);
    // the partial sums live behind the plane's max_blocks if_power values
    // (spectrum mode: no samples to sum -- the launch only carries the call's parameter block to the device)
    kq::launch_block_energy_sum(b->stream, k.spectrum ? nullptr : k.window + (g.M - 1), g.L, k.spectrum ? 0 : (int)k.nblocks,
                                k.pl.if_power + b->cfg.max_blocks,
                                b->stage_host[slot], b->osc_dev2[pp],
                                k.nret ? k.ret_off + k.nret * sizeof(int) : 8 * k.Cmax * sizeof(double) + k.nblocks,
                                k.spectrum ? nullptr : k.paired, (int)(g.M - 1), k.steady ? b->osc_dev2[pp ^ 1] : nullptr, (unsigned)k.C,
                                (unsigned)k.Cmax, (double)(k.n_w - b->planes_n_w), (double)(b->out_abs - b->planes_out_abs),
                                // the channels retuned since the last call: their planes, staged by the host, written by a
                                // few more workgroups of the same launch (the advancing threads skip those channels)
                                b->stage_host[slot] + b->patch_off, k.npatch, b->stage_host[slot] + b->bits_off);
  }
  LAUNCH_CHECK("IF power");
  if (b->timing) {
    KQ_TRY(hipEventRecord(b->stage_t0[slot], b->stream));
    b->stage_timed[slot] = true;
    b->stage_h0[slot] = std::chrono::steady_clock::now();
    b->stage_launch[slot] = b->acc.filter_launches;
  }
  // The IF-power recurrence rides in the first full-spectrum launch of the call (one wave of its first workgroup,
  // kq_full16k.hip) where there is one; KQ_IIR_IN_FILTER=0: as a launch of its own in front of the demodulators, as before
  static bool const iir_in_filter_off = getenv("KQ_IIR_IN_FILTER") && atoi(getenv("KQ_IIR_IN_FILTER")) == 0;
  k.iir_off = iir_in_filter_off;
  launch_filter(b, k);
  LAUNCH_CHECK("pre-detection filter");
  b->acc.filter_launches++;
  b->acc.channel_blocks += (uint64_t)k.C * k.nblocks;
  KQ_TRY(hipEventRecord(b->stage_ev[slot], b->stream));
  if (b->timing) b->stage_submit_ms[slot] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b->stage_h0[slot]).count();
  return 0;
}

// Step 5.  The demodulators and what follows them, on the main stream or on their own.
int launch_demodulators(kq_bank *b, Call &k) {
  kq::Geom const &g = b->g;
  int const pp = k.pp, nblocks = (int)k.nblocks;
  kq::Planes const &pl = k.pl;
  kq::ChanDev const &chd = k.chd;
  // Where the demodulators of this call run.  On a second stream they overlap the next call's filter pass -- but that
  // kernel leaves no room beside it (500 of a SIMD's 512 registers), so what they take it loses, and at N = 65536 a
  // displaced sibling workgroup stalls the three that wait for it.  Measured on one box (tools/ab_env_rows.sh,
  // tools/ab_hostio.sh; ms per step overlapped / not): cfg 4 1.432 / 1.432-1.439, pruned 0.821 / 0.819, cfg 2 0.475 /
  // 0.469, cfg 5 1.31 / 1.15 -- but cfg 3 1.464 / 1.488 (the AGC recurrence of an AM or SSB channel is one long thin wave)
  // and, with the planes streamed to the host after every call, 1.54 / 1.60-1.76 (the copy kernel then has the whole next
  // filter pass to hide under).  KQ_DEMOD_OVERLAP=0 / 1 forces either.
  bool const agc_channels = !b->list_host[1].empty() || !b->list_host[2].empty();
  // (round 5, cfg 2 with its fused FM demodulator: overlapped 0.4175-0.4196 ms per step against 0.4194-0.4195 on one box,
  //  0.4427 against 0.4475 on a slower one, with the filter launch itself 9 % longer -- left where it is)
  bool const overlap = b->stream2 != b->stream &&
                       (b->overlap_mode == 1 || (b->overlap_mode < 0 && !b->use64k && (b->pulled_since_call || agc_channels)));
  b->pulled_since_call = false;
  hipStream_t const ds = overlap ? b->stream2 : b->stream;
  int const prev = pp ^ 1;
  if (overlap)
    KQ_TRY(hipStreamWaitEvent(ds, b->stage_ev[k.slot], 0));  // behind this call's filter, hence behind the last call's demodulators if they ran on the main stream
  else if (b->calls > 0 && b->demod_overlapped[prev])
    KQ_TRY(hipStreamWaitEvent(ds, b->ev_demod_done[prev], 0));  // the channel state they carry
  if (b->out_pending) {  // kq_bank_pull_planes_async is still reading the audio / status planes of the last call
    KQ_TRY(hipStreamWaitEvent(ds, b->pull_done[(b->pulls - 1) % kq_bank::kPullRing], 0));
    b->out_pending = false;
  }
  // the IF-power recurrence over the call's blocks: one wave, consumed by the demodulators only.  Where the call has a
  // full-spectrum launch it has ridden in that (iir_arm above: -5..6 us per step at cfg 4 and cfg 5, the filter kernel's own
  // time unchanged; tools/ab_libs.sh against the commit before); otherwise it runs here, with the demodulators and
  // not in front of the filter (folded into the sum's launch -- its last workgroup taking tagged partial sums as they
  // arrive -- it saved nothing measurable: 1.422 against 1.421 ms per step; on the second stream beside the filter pass,
  // with an event each way, it cost 7-9 us per step where the demodulators run on the main stream -- a wait on another
  // queue's event is dearer than the 6.5 us kernel: cfg 2 0.4326 -> 0.4416, cfg 4 1.5050 -> 1.5124, tools/ab_env.sh)
  // the control plane's demodulator-side writes, on the stream this call's demodulators run on, in front of them
  if (ctl_flush(b, CTL_DEMOD, ds)) return -1;
  if (k.spectrum)  // the IF power belongs to whoever fed the master (radio.c:123,143-145): status.if_power = 0, not what a
                   // normal call two calls back left in this parity's plane
    KQ_TRY(hipMemsetAsync(pl.if_power, 0, k.nblocks * sizeof(float), ds));
  else if (!k.iir_done)
    kq::launch_block_energy_iir(ds, pl.if_power + b->cfg.max_blocks, g.L, nblocks,
                                reinterpret_cast<const unsigned char *>(b->osc_dev2[pp] + 8 * k.Cmax), b->energy_state, pl.if_power);
  {
    Scope t(b, 1, ds);
    int const nfm = (int)b->list_host[0].size(), nam = (int)b->list_host[1].size(), nlin = (int)b->list_host[2].size();
    bool const fused_fm = kq::demod64_supported(g);  // else: wave-per-channel AM / linear, generic FM
    kq::launch_demod64(ds, g, chd, pl, b->list_dev[0], fused_fm ? nfm : 0, b->list_dev[1], nam, b->list_dev[2], nlin, nblocks,
                       b->cfg.compute_n0);
    if (!fused_fm) {
      kq::launch_demod_fm(ds, g, chd, pl, b->tw, b->list_dev[0], nfm, nblocks, b->cfg.compute_n0, b->fmout,
                          b->fm_hist[b->fm_hist_cur], b->fm_hist[b->fm_hist_cur ^ 1]);
      if (nfm > 0) b->fm_hist_cur ^= 1;
    }
  }
  LAUNCH_CHECK("demodulators");
  if (!b->list_pll_host.empty())
    kq::launch_demod_pll(ds, g, chd, pl, b->tw, b->list_pll_dev, (int)b->list_pll_host.size(), b->pll_chunks_dev, b->pll_slot_dev,
                         nblocks, b->cfg.compute_n0);
  if (g.pl_n > 0 && !b->list_host[0].empty())
    kq::launch_pl_track(ds, g, chd, pl, b->tw, b->list_dev[0], (int)b->list_host[0].size(), nblocks);
  if (b->pcm_on) {
    ChanList const act = active_channels(b, b->list_active_ds_dev);
    kq::launch_pcm(ds, g, pl, b->pcm, b->pcm_mask, act.n, nblocks, act.list);
  }
  if (overlap) KQ_TRY(hipEventRecord(b->ev_demod_done[pp], ds));
  b->demod_overlapped[pp] = overlap;
  LAUNCH_CHECK("PLL / PL tone / PCM stage");
  return 0;
}

// Step 6.  The host's bookkeeping moves on by the call's blocks.
void advance_bookkeeping(kq_bank *b, Call const &k) {
  kq::Geom const &g = b->g;
  unsigned const nblocks = k.nblocks;
  b->pl = k.pl;  // what the pull functions read
  b->calls++;
  b->planes_n_w = k.n_w;  // what this parity's planes on the device describe
  b->planes_out_abs = b->out_abs;
  b->n_abs += (int64_t)nblocks * g.L;
  b->out_abs += (int64_t)nblocks * g.olen;
  for (int c : b->patch_list)
    if ((size_t)c < b->chans.size()) b->chans[c].patched = false;
  b->patch_list.clear();
  // the channels that went through this call with samples of an old oscillator in their windows: the call has moved the
  // windows on by nblocks L; whoever has old samples left (M - 1 > L and a short call) goes through the next call the same way
  for (int c : b->ret_host) {
    if ((size_t)c >= b->chans.size()) continue;
    HostChan &h = b->chans[c];
    if (!h.retuned) continue;
    h.hist_old -= (int64_t)nblocks * g.L;
    for (int64_t &n : h.hist_oldx) n = std::max<int64_t>(0, n - (int64_t)nblocks * g.L);
    if (h.hist_old > 0 && h.active) {
      note_patch(b, c);
    } else {
      h.retuned = false;
      h.hist_old = 0;
      for (int64_t &n : h.hist_oldx) n = 0;
    }
  }
  b->ret_host.clear();
  if (!k.steady) {
    for (HostChan &h : b->chans) {
      h.lo2.rebase(b->n_abs);
      h.dop.rebase(b->n_abs);
      h.shift.rebase(b->out_abs);
    }
    b->rebased_at = b->n_abs;
    b->osc_dirty = k.spectrum != nullptr;  // (a spectrum call stages no oscillators the next call could advance)
  }  // (steady calls keep the host's closed forms fresh a few channels at a time: the rolling re-reference above)
  b->last_blocks = nblocks;
}

// The kernels of one call over `nblocks` blocks whose first window starts at `window`
// `spectrum` != null: the master's transform has been done elsewhere (execute_filter_input of the compat surface) and
// `spectrum` holds its N bins per block -- slave, compute_n0 and demodulators only (kq_bank_process_spectrum)
int run_blocks_timed(kq_bank *b, const float2 *window, unsigned nblocks, const unsigned char *update_host,
                     const float2 *spectrum) {
  Call k{window, nblocks, update_host, spectrum, (int)b->chans.size(), b->cfg.max_channels};
  if (decide_sweeps(b, k) || stage_history(b, k) || choose_filter_variant(b, k) || launch_energy_and_filter(b, k) ||
      launch_demodulators(b, k))
    return -1;
  advance_bookkeeping(b, k);
  return (int)nblocks;
}

// kq_bank_get_host_timing: the host's wall time inside one call, kernels only queued (call_ms includes slot_wait_ms)
int run_blocks(kq_bank *b, const float2 *window, unsigned nblocks, const unsigned char *update_host,
               const float2 *spectrum = nullptr) {
  auto const t0 = std::chrono::steady_clock::now();
  int const rc = run_blocks_timed(b, window, nblocks, update_host, spectrum);
  // A call that failed may have left the lists' bulk records queued and unapplied; a 4-byte record of lists_add /
  // lists_remove beside them in one launch would race with the chunk that covers it.  With the lists marked
  // stale those entry points queue nothing, and the next call's rebuild rewrites the queued chunks in place.
  if (rc < 0) b->lists_dirty = true;
  b->host_acc.call_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  b->host_acc.calls++;
  return rc;
}

// The back-pressure wait of a process call (the staging slot it is about to fill was last read four calls ago), taken
// BEFORE the call looks at any state and with the handle's lock let go: the operator's thread is not kept out for the
// length of a device wait (tools/soak_realtime.py showed 10 ms set_filter calls that were this wait).  Only the
// receiver thread advances stage_next, so the slot is still the next one when the lock is back.
int slot_prewait(BankScope &scope, kq_bank *b) {
  hipEvent_t const ev = b->stage_ev[b->stage_next];
  auto const t0 = std::chrono::steady_clock::now();
  {
    Unlocked u(scope);
    KQ_TRY(hipEventSynchronize(ev));
  }
  double const w = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  b->host_acc.slot_wait_ms += w;
  b->host_acc.call_ms += w;
  return 0;
}

}  // namespace

extern "C" {

unsigned kq_bank_blocks_ready(const kq_bank *b) {
  if (!b) return 0;
  LockOnly lk(b);
  return (unsigned)(b->pending / b->g.L);
}


int kq_bank_process(kq_bank *b) {
  BankScope dev_scope_(b, true);
  if (!b) {
    kq_internal_set_error("NULL bank");
    return -1;
  }
  if (slot_prewait(dev_scope_, b)) return -1;
  kq::Geom const &g = b->g;
  if (acc_flush(b)) return -1;  // what kq_bank_push_rtp has gathered goes into the ring now
  unsigned nb = (unsigned)(b->pending / g.L);
  if (nb > b->cfg.max_blocks) nb = b->cfg.max_blocks;
  if (nb == 0) return 0;
  std::vector<unsigned char> upd(nb);
  for (unsigned i = 0; i < nb; i++) upd[i] = b->zero_tail[i] ? 0 : 1;
  int const done = run_blocks(b, b->ring[b->cur], nb, upd.data());
  if (done < 0) return -1;
  b->zero_tail.erase(b->zero_tail.begin(), b->zero_tail.begin() + nb);
  // overlap-save history (filter.c:164) plus any unprocessed tail moves to the other ring buffer
  size_t const consumed = (size_t)nb * g.L;
  size_t const keep = (size_t)(g.M - 1) + (b->pending - consumed);
  KQ_TRY(hipMemcpyAsync(b->ring[b->cur ^ 1], b->ring[b->cur] + consumed, keep * sizeof(float2), hipMemcpyDeviceToDevice,
                         b->stream));
  b->cur ^= 1;
  b->pending -= consumed;
  return done;
}

int kq_bank_process_resident(kq_bank *b, const void *iq_dev, unsigned nblocks) {
  BankScope dev_scope_(b, true);
  if (!b || !iq_dev) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  if (nblocks == 0 || nblocks > b->cfg.max_blocks) {
    kq_internal_set_error("nblocks %u out of range 1..%u", nblocks, b->cfg.max_blocks);
    return -1;
  }
  if (slot_prewait(dev_scope_, b)) return -1;
  std::vector<unsigned char> upd(nblocks, 1);
  return run_blocks(b, (const float2 *)iq_dev, nblocks, upd.data());
}

int kq_bank_process_spectrum(kq_bank *b, const void *spectrum_dev, unsigned nblocks) {
  BankScope dev_scope_(b, true);
  if (!b || !spectrum_dev) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  if (nblocks == 0 || nblocks > b->cfg.max_blocks) {
    kq_internal_set_error("nblocks %u out of range 1..%u", nblocks, b->cfg.max_blocks);
    return -1;
  }
  for (HostChan const &h : b->chans) {
    if (!h.active) continue;
    // the spectrum is what it is: a channel that still has an oscillator to apply cannot be served from it
    if (h.lo2.set_f != 0 || h.dop.set_f != 0) {
      kq_internal_set_error("kq_bank_process_spectrum: a channel has a second LO or Doppler set; the mix belongs in front of the master");
      return -1;
    }
  }
  std::vector<unsigned char> upd(nblocks, 0);
  return run_blocks(b, nullptr, nblocks, upd.data(), (const float2 *)spectrum_dev);
}

}  // extern "C"
