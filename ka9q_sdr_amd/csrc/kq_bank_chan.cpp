// kq_bank_chan.cpp -- channels coming, going and changing: the carrier loops' slots (pll_*), what a configuration is
// refused for, kq_bank_add_channel(s), _remove_channel, _set_mode, _set_linear_options, the oscillator setters, _set_n0,
// _set_filter, _channel_active, _num_channels.  None of it touches the device but kq_bank_add_channels' batched path and the
// allocation of carrier-loop chunks: the changes gather in the control queues (kq_bank_ctl.cpp) for the next call.
// Lock: every entry point takes it through BankScope, kq_bank_channel_active and _num_channels through LockOnly; none lets
// go of it (the batched add waits for the device with the lock held: set-up, not steady state).  The file-local functions
// want it held by the caller.
#include "kq_bank.hpp"

using namespace kq::bank;

namespace {

// the slave's output type (filter.h: independent sidebands come out as the cross-conjugate pair)
int out_type_of(const kq_channel_config &k) { return (k.demod_type == KQ_LINEAR_DEMOD && k.isb) ? kq::FT_CROSS_CONJ : kq::FT_COMPLEX; }
bool is_pll(const kq_channel_config &c) { return c.demod_type == KQ_LINEAR_DEMOD && c.pll; }

// checks before a channel becomes a PLL channel (linear.c:51-56: the carrier search window is +-300 Hz, x2 when squaring,
// in bins of the 65536-point transform)
int pll_admit(kq_bank *b, const kq_channel_config &m) {
  float const samptime = (float)b->g.D / (float)b->g.samprate;
  float const binsize = (float)(1. / (65536 * samptime));
  int const nbins = 2 * (int)round((m.square ? 2 : 1) * 300.f / binsize) + 1;
  if (nbins > 4096) {
    kq_internal_set_error("output rate too low for the PLL search window (%d bins > 4096)", nbins);
    return -1;
  }
  return 0;
}

// A slot for channel c's carrier loop, started afresh (linear.c:97-112): state and ring are zeroed by fill records of the
// demodulator side's queue -- applied in front of the next call's demodulators, behind the ones in flight, which may
// still be running the slot's previous owner.  Nothing here waits for the device; a chunk of slots is allocated when the
// free list runs out (33 MiB per 64 channels).
int pll_acquire(kq_bank *b, int c) {
  size_t const Cmax = b->cfg.max_channels;
  if (!b->list_pll_dev) {
    if (alloc_cleared(b, &b->list_pll_dev, Cmax) || alloc_cleared(b, &b->pll_slot_dev, Cmax) ||
        alloc_cleared(b, &b->pll_chunks_dev, (size_t)kq_bank::kMaxPllChunks))
      return -1;
  }
  if (b->pll_free.empty()) {
    if ((int)b->pll_chunks.size() >= kq_bank::kMaxPllChunks) {
      kq_internal_set_error("at most %d carrier-tracking (pll) channels per bank", kq_bank::kMaxPllChunks * kq::kPllChunk);
      return -1;
    }
    kq::PllChunk ck{};
    if (alloc_cleared(b, &ck.state, (size_t)kq::kPllChunk) || alloc_cleared(b, &ck.rings, (size_t)kq::kPllChunk * 65536) ||
        alloc_cleared(b, &ck.side, (size_t)kq::kPllChunk * 4096)) {
      b->release(&ck.state, &ck.rings, &ck.side);
      return -1;
    }
    int const k = (int)b->pll_chunks.size();
    b->pll_chunks.push_back(ck);
    if (ctl_put(b, CTL_DEMOD, b->pll_chunks_dev + k, &ck, sizeof ck)) return -1;
    for (int s = kq::kPllChunk - 1; s >= 0; s--) b->pll_free.push_back(k * kq::kPllChunk + s);
  }
  int const slot = b->pll_free.back();
  b->pll_free.pop_back();
  kq::PllChunk const &ck = b->pll_chunks[slot / kq::kPllChunk];
  int const sl = slot % kq::kPllChunk;
  if (ctl_fill(b, CTL_DEMOD, ck.state + sl, 0u, sizeof(kq::PllState)) ||
      ctl_fill(b, CTL_DEMOD, ck.rings + (size_t)sl * 65536, 0u, sizeof(float2) * 65536) ||
      ctl_put(b, CTL_DEMOD, b->pll_slot_dev + c, &slot, sizeof(int))) {
    b->pll_free.push_back(slot);
    return -1;
  }
  b->chans[c].pll_slot = slot;
  return 0;
}
void pll_release(kq_bank *b, int c) {
  int &slot = b->chans[c].pll_slot;
  if (slot >= 0) b->pll_free.push_back(slot);
  slot = -1;
}

// what kq_bank_add_channel(s) and kq_bank_set_mode refuse in a channel configuration (`entry`: its index in a batch, or -1)
int check_channel_config(const kq_bank *b, const kq_channel_config &k, int entry = -1) {
  char at[32] = "";
  if (entry >= 0) snprintf(at, sizeof at, " (entry %d)", entry);
  if (k.demod_type < KQ_LINEAR_DEMOD || k.demod_type > KQ_FM_DEMOD) {
    kq_internal_set_error("unknown demod_type %d%s", k.demod_type, at);
    return -1;
  }
  if (std::isnan(k.low) || std::isnan(k.high)) {  // filter.c:504-505
    kq_internal_set_error("NaN filter edge%s", at);
    return -1;
  }
  if (k.demod_type == KQ_FM_DEMOD && !kq::demod64_supported(b->g) && kq::demod_fm_lds_bytes(b->g) > 160 * 1024) {
    // the FM kernels keep one block of samples / the N/D-point audio master in LDS (N/D <= 8192)
    kq_internal_set_error("FM working set of %zu bytes exceeds the 160 KiB of LDS at this geometry", kq::demod_fm_lds_bytes(b->g));
    return -1;
  }
  return 0;
}

// oscillator setter scalings: radio.c:299, radio.c:182, radio.c:309
void set_oscillators(const kq_bank *b, HostChan &h, const kq_channel_config &k) {
  double const fs = b->g.samprate;
  h.lo2.set(k.second_lo == 0 ? 0.0 : k.second_lo / fs, 0.0, b->n_abs);
  h.dop.set(-k.doppler / fs, -k.doppler_rate / (fs * fs), b->n_abs);
  h.shift.set(k.shift == 0 ? 0.0 : k.shift * b->g.D / fs, 0.0, b->out_abs);
}

}  // namespace

extern "C" {

int kq_bank_add_channel(kq_bank *b, const kq_channel_config *cfg) {
  BankScope dev_scope_(b);
  if (!b || !cfg) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  // the lowest hole a removed channel left, else a new slot at the end
  int c = (int)b->chans.size();
  for (int k = 0; k < (int)b->chans.size(); k++)
    if (!b->chans[k].active) {
      c = k;
      break;
    }
  if ((size_t)c >= b->cfg.max_channels) {
    kq_internal_set_error("bank is full (%u channels)", b->cfg.max_channels);
    return -1;
  }
  if (check_channel_config(b, *cfg)) return -1;
  if (is_pll(*cfg) && pll_admit(b, *cfg)) return -1;
  HostChan h;
  h.cfg = *cfg;
  h.out_type = out_type_of(*cfg);
  set_oscillators(b, h, *cfg);
  bool const appended = c == (int)b->chans.size();
  if (appended)
    b->chans.push_back(h);
  else
    b->chans[c] = h;
  if ((is_pll(*cfg) && pll_acquire(b, c)) || upload_channel(b, c) || queue_design(b, c)) {
    pll_release(b, c);  // (the slot it may have been given)
    release_n0slot(b, b->chans[c].n0slot);  // (the mask set it may have been given)
    b->chans[c].n0slot = -1;
    if (appended)
      b->chans.pop_back();
    else
      b->chans[c].active = false;
    return -1;
  }
  if (lists_add(b, c)) return -1;
  b->chan_tw_dirty = true;
  b->row_ph_dirty = true;
  // a channel more leaves the steady state of the others alone: its planes are patched in by the next call
  b->chans[c].r_eff = 0;
  b->n_active++;
  b->cache_any = true;
  b->sweep_lists_dirty = true;
  note_patch(b, c);
  return c;
}

// Many channels at once (a receiver bank of tens of thousands of channels is set up in one go): the same result as
// kq_bank_add_channel called n times, but every distinct response is designed once (one launch for all of them), every
// distinct compute_n0 mask is built once, and each per-channel plane is uploaded with one copy instead of n.
int kq_bank_add_channels(kq_bank *b, const kq_channel_config *cfgs, unsigned n, int *indices) {
  BankScope dev_scope_(b);
  if (!b || (!cfgs && n)) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  if (n == 0) return 0;
  bool holes = false, any_pll = false, any_nan = false;
  for (HostChan const &h : b->chans) holes = holes || !h.active;
  for (unsigned i = 0; i < n; i++) any_pll = any_pll || is_pll(cfgs[i]);
  // a NaN beta is not a key the ordered maps below can hold (it breaks their strict weak ordering): such a batch takes
  // the one-by-one path, whose design takes the value as the reference's does (queue_design)
  for (unsigned i = 0; i < n; i++) any_nan = any_nan || std::isnan(cfgs[i].kaiser_beta);
  if (holes || any_pll || any_nan || n < 4) {  // slot reuse and carrier-loop slots: one by one; all or nothing
    std::vector<int> got;
    for (unsigned i = 0; i < n; i++) {
      int const c = kq_bank_add_channel(b, &cfgs[i]);
      if (c < 0) {
        std::string const why = kq_last_error();
        for (size_t k = got.size(); k-- > 0;) (void)kq_bank_remove_channel(b, got[k]);
        kq_internal_set_error("%s", why.c_str());
        return -1;
      }
      got.push_back(c);
      if (indices) indices[i] = c;
    }
    return (int)n;
  }
  kq::Geom const &g = b->g;
  size_t const c0 = b->chans.size();
  if (c0 + n > b->cfg.max_channels) {
    kq_internal_set_error("bank is full (%u channels): %zu present, %u more asked for", b->cfg.max_channels, c0, n);
    return -1;
  }
  for (unsigned i = 0; i < n; i++)
    if (check_channel_config(b, cfgs[i], (int)i)) return -1;
  // responses: every distinct (out_type, edges, beta) once, one launch per out_type
  std::vector<HostChan> hs(n);
  struct Key {
    float lo, hi, beta;
    bool operator<(Key const &o) const { return lo != o.lo ? lo < o.lo : hi != o.hi ? hi < o.hi : beta < o.beta; }
  };
  for (int ot : {(int)kq::FT_COMPLEX, (int)kq::FT_CROSS_CONJ}) {
    std::map<Key, int> job;
    std::vector<kq::BandEdges> edges;
    std::vector<int> which(n, -1);
    for (unsigned i = 0; i < n; i++) {
      kq_channel_config const &k = cfgs[i];
      if (out_type_of(k) != ot) continue;
      float lo_n, hi_n;
      design_edges(g, k, false, &lo_n, &hi_n);  // (as queue_design)
      Key const key{lo_n, hi_n, k.kaiser_beta};
      auto it = job.find(key);
      if (it == job.end()) {
        it = job.emplace(key, (int)edges.size()).first;
        edges.push_back(kq::BandEdges{lo_n, hi_n, k.kaiser_beta});
      }
      which[i] = it->second;
    }
    if (edges.empty()) continue;
    std::vector<kq::cfloat> resp;
    std::vector<float> ng;
    if (kq::design_responses(g.N, g.olen, g.Mdec, ot, edges, resp, ng) || resp.size() != edges.size() * (size_t)g.Ndec) {
      kq_internal_set_error("response design failed");
      return -1;
    }
    for (unsigned i = 0; i < n; i++)
      if (which[i] >= 0) {
        hs[i].out_type = ot;
        hs[i].resp.assign(resp.begin() + (size_t)which[i] * g.Ndec, resp.begin() + (size_t)(which[i] + 1) * g.Ndec);
        hs[i].noise_gain = ng[which[i]];
      }
  }
  std::map<float, std::vector<kq::cfloat>> aresp_by_beta;  // fm.c:54-66 depends on the geometry and beta only
  for (unsigned i = 0; i < n; i++) {
    kq_channel_config const &k = cfgs[i];
    HostChan &h = hs[i];
    h.cfg = k;
    set_oscillators(b, h, k);
    if (k.demod_type == KQ_FM_DEMOD && !k.flat) {
      auto it = aresp_by_beta.find(k.kaiser_beta);
      if (it == aresp_by_beta.end()) {
        std::vector<kq::cfloat> a = kq::design_fm_audio_response(g.olen, g.Mdec, g.dsamprate, k.kaiser_beta);
        if (a.empty()) {
          kq_internal_set_error("FM audio response design failed");
          return -1;
        }
        it = aresp_by_beta.emplace(k.kaiser_beta, std::move(a)).first;
      }
      h.aresp = it->second;
    }
  }
  if (ctl_flush_now(b) || sync_all(b)) return -1;  // (what the control plane has queued goes first: the copies below are immediate)
  // per-channel planes of the new range, one copy each
  auto put = [&](auto *dst, auto const &v) -> int {
    KQ_TRY(hipMemcpy(dst + c0, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
    return 0;
  };
  {
    std::vector<int> mode(n), flags(n), hangmax(n);
    std::vector<float> low(n), high(n), fm_gain(n), headroom(n), recovery(n), gain(n), ngain(n), nanv(n, NAN);
    std::vector<float2> one(n, make_float2(1.f, 0.f));  // fm.c:26
    for (unsigned i = 0; i < n; i++) {
      Derived const d = derive(g, cfgs[i]);
      mode[i] = d.mode;
      flags[i] = d.flags;
      hangmax[i] = d.hangmax;
      low[i] = cfgs[i].low;
      high[i] = cfgs[i].high;
      fm_gain[i] = d.fm_gain;
      headroom[i] = cfgs[i].headroom;
      recovery[i] = d.recovery;
      gain[i] = d.init_gain;
      ngain[i] = hs[i].noise_gain;
    }
    if (put(b->chd.mode, mode) || put(b->chd.flags, flags) || put(b->chd.fflags, flags) || put(b->chd.hangmax, hangmax) || put(b->chd.low, low) ||
        put(b->chd.high, high) || put(b->chd.fm_gain, fm_gain) || put(b->chd.headroom, headroom) ||
        put(b->chd.recovery, recovery) || put(b->chd.gain, gain) || put(b->chd.noise_gain, ngain) || put(b->chd.n0, nanv) ||
        put(b->chd.plfreq, nanv) || put(b->chd.fm_state, one))
      return -1;
  }
  // demodulator state at its prologue values (fm.c:26,68-69; am.c:26,33; linear.c:33)
  KQ_TRY(hipMemset(b->chd.lastaudio + c0, 0, n * sizeof(float)));
  KQ_TRY(hipMemset(b->chd.sq_count + c0, 0, n * sizeof(int)));
  KQ_TRY(hipMemset(b->chd.hang + c0, 0, n * sizeof(int)));
  KQ_TRY(hipMemset(b->chd.dc + c0, 0, n * sizeof(float)));
  KQ_TRY(hipMemset(b->chd.foffset + c0, 0, n * sizeof(float)));
  KQ_TRY(hipMemset(b->chd.pdev + c0, 0, n * sizeof(float)));
  if (g.Mdec > 1) {
    size_t const w = (size_t)(g.Mdec - 1);
    KQ_TRY(hipMemset(b->chd.ahist + c0 * w, 0, n * w * sizeof(float)));
    for (int k = 0; k < 2; k++)
      if (b->fm_hist[k]) KQ_TRY(hipMemset(b->fm_hist[k] + c0 * w, 0, n * w * sizeof(float)));
  }
  if (g.pl_n > 0) {
    KQ_TRY(hipMemset(b->chd.plring + c0 * 16384, 0, (size_t)n * 16384 * sizeof(float)));
    KQ_TRY(hipMemset(b->chd.pl_ptr + c0, 0, n * sizeof(*b->chd.pl_ptr)));
    KQ_TRY(hipMemset(b->chd.pl_last + c0, 0, n * sizeof(*b->chd.pl_last)));
  }
  {  // responses
    std::vector<float2> resp((size_t)n * g.Ndec);
    for (unsigned i = 0; i < n; i++) memcpy(&resp[(size_t)i * g.Ndec], hs[i].resp.data(), sizeof(float2) * g.Ndec);
    KQ_TRY(hipMemcpy(b->chd.resp + c0 * g.Ndec, resp.data(), resp.size() * sizeof(float2), hipMemcpyHostToDevice));
    size_t const na = (size_t)g.Ndec / 2 + 1;
    std::vector<float2> ar((size_t)n * na, make_float2(0.f, 0.f));
    bool any = false;
    for (unsigned i = 0; i < n; i++)
      if (!hs[i].aresp.empty()) {
        memcpy(&ar[(size_t)i * na], hs[i].aresp.data(), sizeof(float2) * na);
        any = true;
      }
    if (any) KQ_TRY(hipMemcpy(b->chd.aresp + c0 * na, ar.data(), ar.size() * sizeof(float2), hipMemcpyHostToDevice));
  }
  if (b->chd.n0lane) {  // compute_n0's lane masks: one set per distinct pair of edges, shared
    int const nsub = b->use64k ? 4 : 1;
    std::vector<int> slots(n);
    unsigned taken = 0;
    auto fill = [&]() -> int {
      for (unsigned i = 0; i < n; i++) {
        bool fresh = false;
        int const slot = acquire_n0slot(b, cfgs[i].low, cfgs[i].high, &fresh);
        hs[i].n0slot = slots[i] = slot;
        if (slot < 0) return -1;
        taken = i + 1;
        if (fresh) {
          std::vector<unsigned long long> m;
          std::vector<unsigned> meta;
          build_n0mask(b, cfgs[i].low, cfgs[i].high, m, meta);
          KQ_TRY(hipMemcpy(b->chd.n0lane + (size_t)slot * nsub * 256, m.data(), m.size() * sizeof(m[0]), hipMemcpyHostToDevice));
          KQ_TRY(hipMemcpy(b->chd.n0meta + (size_t)slot * nsub, meta.data(), meta.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        }
      }
      KQ_TRY(hipMemcpy(b->chd.n0slot + c0, slots.data(), n * sizeof(int), hipMemcpyHostToDevice));
      return 0;
    };
    if (fill()) {  // all or nothing: the references taken so far go back
      for (unsigned i = 0; i < taken; i++) release_n0slot(b, slots[i]);
      return -1;
    }
  }
  for (unsigned i = 0; i < n; i++) {
    b->chans.push_back(std::move(hs[i]));
    if (indices) indices[i] = (int)(c0 + i);
  }
  b->lists_dirty = true;
  b->osc_dirty = true;
  b->chan_tw_dirty = true;
  b->row_ph_dirty = true;
  return (int)n;
}

// close_chan equivalent: the demodulator thread is joined and its struct demod freed (radio.c:335-337 does the join
// for a mode change).  Channel numbers of the others do not change; the slot is a hole until an add reuses it.
int kq_bank_remove_channel(kq_bank *b, int ch) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch)) {
    kq_internal_set_error("bad channel");
    return -1;
  }
  HostChan &h = b->chans[ch];
  pll_release(b, ch);  // (a carrier loop's slot goes back on the free list: its next owner starts it afresh)
  // (nothing on the device changes: the calls in flight still carry the channel, the next call's lists do not)
  if (lists_remove(b, ch)) return -1;
  h.active = false;
  h.retuned = false;
  h.hist_old = 0;
  for (int64_t &n : h.hist_oldx) n = 0;
  h.patched = false;  // (its entry on the patch list, if any, is skipped: the next call stages the whole bank)
  release_n0slot(b, h.n0slot);
  h.n0slot = -1;
  // (the others' steady state is untouched: the launch decisions' counters lose this channel, the lists are redone)
  b->n_active--;
  b->n_swept -= h.r_eff != 0;
  b->n_fast -= std::fabs(h.r_eff) > sweep_limit(b);
  b->cache_any = b->n_active > 0;
  b->sweep_lists_dirty = true;
  h.r_eff = 0;
  h.lo2 = h.dop = h.shift = h.lo2_old = h.dop_old = Osc{};
  for (int l = 0; l < kq::kOldLevels; l++) h.lo2_oldx[l] = h.dop_oldx[l] = Osc{};
  h.out_rtp = kq_out_rtp_state{};
  while (!b->chans.empty() && !b->chans.back().active) b->chans.pop_back();  // holes at the end just go
  return 0;
}

int kq_bank_channel_active(const kq_bank *b, int ch) {
  if (!b) return 0;
  LockOnly lk(b);
  return valid_ch(b, ch) ? 1 : 0;
}

unsigned kq_bank_num_channels(const kq_bank *b) {
  if (!b) return 0;
  LockOnly lk(b);
  return (unsigned)b->chans.size();
}

int kq_bank_set_mode(kq_bank *b, int ch, const kq_channel_config *m) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !m) {
    kq_internal_set_error("bad channel or NULL mode");
    return -1;
  }
  if (check_channel_config(b, *m)) return -1;
  // pthread_join of the old demodulator thread (radio.c:335-337): the new state is written on the main stream behind the
  // last call's demodulators (upload_channel); only carrier-loop slots, moved by synchronous copies, need the device idle
  HostChan &h = b->chans[ch];
  bool const was = is_pll(h.cfg), now = is_pll(*m);
  if (now && pll_admit(b, *m)) return -1;
  {  // a fresh loop either way (linear.c:97-112).  The new slot is taken BEFORE the old one goes back: a failure (the
     // allocation of another chunk) then leaves the channel as it was, loop and all
    int const old_slot = h.pll_slot;
    if (now) {
      h.pll_slot = -1;
      if (pll_acquire(b, ch)) {
        h.pll_slot = old_slot;
        if (old_slot >= 0 && ctl_put(b, CTL_DEMOD, b->pll_slot_dev + ch, &old_slot, sizeof(int))) return -1;
        return -1;
      }
    }
    if (was && old_slot >= 0) {
      b->pll_free.push_back(old_slot);
      if (!now) h.pll_slot = -1;
    }
  }
  // the mode table entry (radio.c:341-363); the input oscillators are not touched
  h.cfg.demod_type = m->demod_type;
  h.cfg.low = m->low > m->high ? m->high : m->low;  // radio.c:343-349
  h.cfg.high = m->low > m->high ? m->low : m->high;
  h.cfg.flat = m->flat;
  h.cfg.isb = m->isb;
  h.cfg.channels = m->channels;
  h.cfg.pll = m->pll;
  h.cfg.square = m->square;
  h.cfg.recovery_rate = m->recovery_rate;
  h.cfg.hangtime = m->hangtime;
  h.cfg.kaiser_beta = m->kaiser_beta;
  h.cfg.headroom = m->headroom;
  h.cfg.shift = m->shift;
  h.out_type = out_type_of(h.cfg);
  h.shift.set(m->shift == 0 ? 0.0 : m->shift * b->g.D / (double)b->g.samprate, 0.0, b->out_abs);  // radio.c:367
  if (upload_channel(b, ch, false) || queue_design(b, ch)) return -1;
  if (lists_retype(b, ch)) return -1;
  note_patch(b, ch);  // the shift oscillator (radio.c:367)
  return 0;
}

// linear.c:117-120 copies demod->filter.isb into the slave's out_type before every block, and linear.c:291-300 looks
// at demod->output.channels after it: both may change while the demodulator runs, without touching its AGC or the
// response (which keeps the gain it was designed with until the next set_filter, as in the reference).
int kq_bank_set_linear_options(kq_bank *b, int ch, int isb, int channels) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || (channels != 1 && channels != 2)) {
    kq_internal_set_error("bad channel, or channels not 1 or 2");
    return -1;
  }
  HostChan &h = b->chans[ch];
  if (h.cfg.demod_type != KQ_LINEAR_DEMOD) {
    kq_internal_set_error("not a linear channel");
    return -1;
  }
  if ((h.cfg.isb != 0) == (isb != 0) && h.cfg.channels == channels) return 0;
  h.cfg.isb = isb != 0;
  h.cfg.channels = channels;
  h.out_type = out_type_of(h.cfg);
  int const flags = channel_flags(h.cfg);
  // (filter.out->out_type for the slave, demod->output.channels for the hand-off: each side from its next block on)
  if (ctl_put(b, CTL_FILTER, b->chd.fflags + ch, &flags, sizeof(int))) return -1;
  if (ctl_put(b, CTL_DEMOD, b->chd.flags + ch, &flags, sizeof(int))) return -1;
  return 0;
}

int kq_bank_set_second_lo(kq_bank *b, int ch, double hz) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || std::isnan(hz)) {
    kq_internal_set_error("bad channel or NaN");
    return -1;
  }
  note_retune(b, ch);
  b->chans[ch].cfg.second_lo = hz;
  b->chans[ch].lo2.set(hz == 0 ? 0.0 : hz / b->g.samprate, 0.0, b->n_abs);
  b->chan_tw_dirty = true;
  b->row_ph_dirty = true;
  note_patch(b, ch);
  return 0;
}

int kq_bank_set_doppler(kq_bank *b, int ch, double hz, double hz_per_s) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || std::isnan(hz) || std::isnan(hz_per_s)) {
    kq_internal_set_error("bad channel or NaN");
    return -1;
  }
  double const fs = b->g.samprate;
  note_retune(b, ch);
  b->chans[ch].cfg.doppler = hz;
  b->chans[ch].cfg.doppler_rate = hz_per_s;
  b->chans[ch].dop.set(-hz / fs, -hz_per_s / (fs * fs), b->n_abs);
  b->chan_tw_dirty = true;
  b->row_ph_dirty = true;
  note_patch(b, ch);
  return 0;
}

int kq_bank_set_shift(kq_bank *b, int ch, double hz) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || std::isnan(hz)) {
    kq_internal_set_error("bad channel or NaN");
    return -1;
  }
  b->chans[ch].cfg.shift = hz;
  b->chans[ch].shift.set(hz == 0 ? 0.0 : hz * b->g.D / (double)b->g.samprate, 0.0, b->out_abs);
  note_patch(b, ch);
  return 0;
}

int kq_bank_set_n0(kq_bank *b, int ch, float n0) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch)) {
    kq_internal_set_error("bad channel");
    return -1;
  }
  // the demodulators of a call in flight own the state: written behind them, in front of the next call's
  if (ctl_put(b, CTL_DEMOD, b->chd.n0 + ch, &n0, sizeof n0)) return -1;
  return 0;
}

int kq_bank_set_filter(kq_bank *b, int ch, float low, float high, float beta) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch)) {
    kq_internal_set_error("bad channel");
    return -1;
  }
  if (std::isnan(low) || std::isnan(high)) {  // filter.c:504-505
    kq_internal_set_error("NaN filter edge");
    return -1;
  }
  HostChan &h = b->chans[ch];
  h.cfg.low = low;
  h.cfg.high = high;
  h.cfg.kaiser_beta = beta;
  float const fm_gain = (float)((h.cfg.headroom * M_1_PI * b->g.dsamprate) / fabsf(low - high));
  // the new response takes effect from the next call on (filter.c:538-543 swaps it under the mutex between two blocks):
  // queued for that call; the host does not wait
  if (ctl_put(b, CTL_FILTER, b->chd.low + ch, &low, sizeof(float))) return -1;
  if (ctl_put(b, CTL_FILTER, b->chd.high + ch, &high, sizeof(float))) return -1;
  if (ctl_put(b, CTL_DEMOD, b->chd.fm_gain + ch, &fm_gain, sizeof(float))) return -1;
  if (upload_n0mask(b, ch)) return -1;
  return queue_design(b, ch, true);
}

}  // extern "C"
