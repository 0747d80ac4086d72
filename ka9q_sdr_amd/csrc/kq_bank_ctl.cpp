// kq_bank_ctl.cpp -- the control plane's way to the device: the two write queues (ctl_*), the design queue (design_flush,
// queue_design, fetch_response), compute_n0's shared mask slots, the per-channel constants (derive, upload_channel) and the
// channel lists (lists_*, upload_lists).  Nothing here launches a call's kernels; the call applies what has gathered here
// (ctl_flush, kq_bank_call.cpp).
// Lock: no entry points; every function wants the handle's lock held by the caller and never lets go of it.  The two that
// wait for the device do so with the lock held: fetch_response (kq_bank_get_response) and ctl_flush's wait for a buffer
// handed over kDepth flushes ago.
#include "kq_bank.hpp"

namespace kq::bank {

// room for one more record with `bytes` of payload in queue `side`; a full queue is applied early, on the main stream
// behind the demodulators in flight (never in practice: a megabyte of parameters between two calls)
static int ctl_room(kq_bank *b, int side, size_t bytes) {
  kq_bank::CtlQueue &q = b->ctl[side];
  size_t const payload_cap = kq_bank::CtlQueue::kBytes - kq_bank::CtlQueue::kMaxRec * sizeof(CtlRecHost);
  if (bytes > payload_cap) {
    kq_internal_set_error("control-plane write of %zu bytes exceeds the queue", bytes);
    return -1;
  }
  if (q.nrec >= kq_bank::CtlQueue::kMaxRec || q.used + bytes > payload_cap) return ctl_flush_now(b);
  return 0;
}
// An earlier record for the destination `key` gives way to a new one of `bytes`: cancelled where the new one covers it;
// otherwise (an earlier, LARGER fill under a smaller copy -- no caller does that -- would stay in the launch beside the
// copy) what has gathered is applied first
static int ctl_supersede(kq_bank *b, int side, unsigned long long key, size_t bytes) {
  kq_bank::CtlQueue &q = b->ctl[side];
  auto it = q.at.find(key);
  if (it == q.at.end()) return 0;
  CtlRecHost *old = reinterpret_cast<CtlRecHost *>(q.buf[q.cur]) + it->second;
  if (old->nbytes <= bytes) old->nbytes = 0;
  else if (ctl_flush_now(b)) return -1;
  return 0;
}
// the record joins the queue (room: the caller's business)
static void ctl_append(kq_bank::CtlQueue &q, CtlRecHost const &r) {
  memcpy(q.buf[q.cur] + (size_t)q.nrec * sizeof r, &r, sizeof r);
  q.at[r.dst] = q.nrec;
  q.nrec++;
}
// a record without payload: fill 1, a 32-bit fill with `value`; fill 2, a copy from device memory `src`
static int ctl_put_plain(kq_bank *b, int side, void *dst, size_t bytes, unsigned fill, unsigned value, const void *src) {
  unsigned long long const key = (unsigned long long)(uintptr_t)dst;
  if (ctl_supersede(b, side, key, bytes) || ctl_room(b, side, 0)) return -1;
  ctl_append(b->ctl[side], CtlRecHost{key, (unsigned)bytes, fill, value, 0u, (unsigned long long)(uintptr_t)src});
  return 0;
}

// queue a copy of `bytes` (a multiple of 4) from host memory to device memory / a 32-bit fill of device memory.
// A destination that is already in the queue: the earlier record is rewritten in place (same or larger extent) or
// cancelled and replaced (smaller extent) -- every field of the control plane has one destination and one extent, so a
// partial overlap with a different start does not occur.
int ctl_put(kq_bank *b, int side, void *dst, const void *src, size_t bytes) {
  if (bytes == 0) return 0;
  // a long payload (a channel list of a large bank: 128 KiB) as records of 4 KiB: a record is one workgroup's work, and its
  // loads cross the link -- as ONE record a list took a workgroup ~0.25 ms, which the next call's kernels waited for
  size_t const kChunk = 4096;
  if (bytes > kChunk) {
    for (size_t off = 0; off < bytes; off += kChunk)
      if (ctl_put(b, side, static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, std::min(kChunk, bytes - off)))
        return -1;
    return 0;
  }
  kq_bank::CtlQueue &q = b->ctl[side];
  unsigned long long const key = (unsigned long long)(uintptr_t)dst;
  auto it = q.at.find(key);
  if (it != q.at.end()) {
    CtlRecHost *old = reinterpret_cast<CtlRecHost *>(q.buf[q.cur]) + it->second;
    if (!old->fill && old->nbytes >= bytes) {
      memcpy(q.buf[q.cur] + old->payload_off, src, bytes);
      return 0;
    }
  }
  if (ctl_supersede(b, side, key, bytes) || ctl_room(b, side, bytes)) return -1;
  size_t const off = kq_bank::CtlQueue::kMaxRec * sizeof(CtlRecHost) + q.used;
  memcpy(q.buf[q.cur] + off, src, bytes);
  ctl_append(q, CtlRecHost{key, (unsigned)bytes, 0u, 0u, (unsigned)off, 0ull});
  q.used += (bytes + 15) & ~(size_t)15;
  return 0;
}
int ctl_fill(kq_bank *b, int side, void *dst, unsigned value, size_t bytes) {
  return bytes ? ctl_put_plain(b, side, dst, bytes, 1u, value, nullptr) : 0;
}
// queue a copy of `bytes` from device memory `src`, read when the queue is applied
static int ctl_copy_dev(kq_bank *b, int side, void *dst, const void *src, size_t bytes) {
  return ctl_put_plain(b, side, dst, bytes, 2u, 0u, src);
}
// withdraw a queued write to `dst` (something else is going to write there in front of the same call)
static void ctl_cancel(kq_bank *b, int side, void *dst) {
  kq_bank::CtlQueue &q = b->ctl[side];
  auto it = q.at.find((unsigned long long)(uintptr_t)dst);
  if (it == q.at.end()) return;
  (reinterpret_cast<CtlRecHost *>(q.buf[q.cur]) + it->second)->nbytes = 0;
  q.at.erase(it);
}
// withdraw every queued write that starts inside [dst, dst + bytes): a bulk rewrite of that range follows, and the records
// of one launch are applied concurrently (a 4-byte list entry queued earlier must not land beside the chunk covering it)
static void ctl_cancel_range(kq_bank *b, int side, const void *dst, size_t bytes) {
  kq_bank::CtlQueue &q = b->ctl[side];
  unsigned long long const lo = (unsigned long long)(uintptr_t)dst, hi = lo + bytes;
  for (auto it = q.at.begin(); it != q.at.end();) {
    if (it->first >= lo && it->first < hi) {
      (reinterpret_cast<CtlRecHost *>(q.buf[q.cur]) + it->second)->nbytes = 0;
      it = q.at.erase(it);
    } else
      ++it;
  }
}

// the design jobs gathered since the last call: one launch on the main stream
// `ctl_queue` != null: that many write records of the filter side's queue ride in the same launch (*took_records set)
static int design_flush(kq_bank *b, const void *ctl_queue = nullptr, unsigned ctl_records = 0, bool *took_records = nullptr) {
  kq_bank::DesignQueue &d = b->dq;
  if (took_records) *took_records = false;
  if (d.jobs.empty()) return 0;
  int const p = (int)(d.epoch & 1);
  unsigned const n = (unsigned)d.jobs.size();
  if (d.read_set[d.cur]) KQ_TRY(hipEventSynchronize(d.read[d.cur]));  // (kDepth launches ago)
  unsigned char *pin = d.pin[d.cur];
  memcpy(pin, d.jobs.data(), n * sizeof(kq::DesignJob));
  memcpy(pin + kq_bank::DesignQueue::kMax * sizeof(kq::DesignJob), d.targets.data(), n * sizeof(kq::DesignTarget));
  // ng_next[p] was last written two design launches ago; the records that moved those values on ran on the demodulators' stream
  if (d.ng_moved_set[p]) KQ_TRY(hipStreamWaitEvent(b->stream, d.ng_moved[p], 0));
  if (kq::design_launch(b->stream, b->g.olen, b->g.Mdec, reinterpret_cast<const kq::DesignJob *>(pin),
                        reinterpret_cast<const kq::DesignTarget *>(pin + kq_bank::DesignQueue::kMax * sizeof(kq::DesignJob)), n,
                        d.scratch, ctl_queue, ctl_records)) {
    kq_internal_set_error("response design launch failed");
    return -1;
  }
  if (took_records) *took_records = ctl_queue != nullptr && ctl_records > 0;
  KQ_TRY(hipEventRecord(d.read[d.cur], b->stream));
  d.read_set[d.cur] = true;
  d.cur = (d.cur + 1) % kq_bank::DesignQueue::kDepth;
  d.ng_to_record = p;
  d.epoch++;
  d.jobs.clear();
  d.targets.clear();
  d.at.clear();
  return 0;
}

// apply what has gathered in queue `side` with one launch on `st`
int ctl_flush(kq_bank *b, int side, hipStream_t st) {
  kq_bank::CtlQueue &q = b->ctl[side];
  // (the filter side is always applied on the main stream: with design jobs waiting, its records ride in their launch --
  //  nothing a record writes is read or written by a design job, kq_bank::DesignQueue / ctl_cancel see to that)
  bool applied = false;
  if (side == CTL_FILTER && design_flush(b, q.nrec ? q.buf[q.cur] : nullptr, q.nrec, &applied)) return -1;
  if (q.nrec == 0) return 0;
  if (!applied) kq::launch_ctl_apply(st, q.buf[q.cur], (int)q.nrec);
  KQ_TRY(hipEventRecord(q.applied[q.cur], st));
  q.applied_set[q.cur] = true;
  if (side == CTL_DEMOD && b->dq.ng_to_record >= 0) {
    int const p = b->dq.ng_to_record;
    KQ_TRY(hipEventRecord(b->dq.ng_moved[p], st));
    b->dq.ng_moved_set[p] = true;
    b->dq.ng_to_record = -1;
  }
  q.cur = (q.cur + 1) % kq_bank::CtlQueue::kDepth;
  q.nrec = 0;
  q.used = 0;
  q.at.clear();
  // the buffer gathered into next was handed to the device kDepth flushes ago: long applied
  if (q.applied_set[q.cur]) KQ_TRY(hipEventSynchronize(q.applied[q.cur]));
  return 0;
}
// both queues applied now, on the main stream behind the demodulators in flight (for the rare paths that go on to touch
// the device synchronously: carrier-loop slots, batched channel set-up)
int ctl_flush_now(kq_bank *b) {
  if (b->ctl[0].nrec == 0 && b->ctl[1].nrec == 0 && b->dq.jobs.empty()) return 0;
  if (b->calls > 0) {
    int const last = (int)((b->calls - 1) & 1);
    if (b->demod_overlapped[last]) KQ_TRY(hipStreamWaitEvent(b->stream, b->ev_demod_done[last], 0));
  }
  if (ctl_flush(b, CTL_FILTER, b->stream) || ctl_flush(b, CTL_DEMOD, b->stream)) return -1;
  return 0;
}

// compute_n0's passband exclusion (radio.c:405-411) depends only on the channel's filter edges: one bit per bin, as
// 64-bit lane masks in the order k_filter_full16k holds the bins (kq_device.hpp ChanDev::n0lane).  Same arithmetic as
// the reference, int wrap of k * samprate included (radio.c:407,409).  N = 65536: sub-transform r holds bins 4 q + r.
void build_n0mask(const kq_bank *b, float low, float high, std::vector<unsigned long long> &m, std::vector<unsigned> &meta) {
  kq::Geom const &g = b->g;
  int const nsub = b->use64k ? 4 : 1;
  m.assign((size_t)nsub * 256, 0ull);
  meta.assign(nsub, 0u);
  for (int r = 0; r < nsub; r++)
    for (int t = 0; t < 512; t++) {
      int const ka = kq::full16k_bin(t);
      for (int half = 0; half < 2; half++)
        for (int k3 = 0; k3 < 16; k3++) {
          int const n = nsub * (ka + kq::kFull16kHalf * half + 1024 * k3) + r;
          int const k = (n <= g.N / 2) ? n : n - g.N;
          int const prod = (int)((unsigned)k * (unsigned)g.samprate);
          float const f = (float)prod / g.N;
          if (!(f >= low && f <= high)) {
            m[((size_t)r * 8 + (t >> 6)) * 32 + 16 * half + k3] |= 1ull << (t & 63);
            meta[r]++;
          }
        }
    }
}

// the mask set for these edges: an existing one, or a free slot filled now (*fresh).  Takes a reference.  -1: no slot
// left (cannot happen while every reference belongs to a channel and a channel gives its old slot back BEFORE it asks
// for a new one -- upload_n0mask; the planes hold exactly max_channels sets, so a slot past them is refused, never
// written)
int acquire_n0slot(kq_bank *b, float low, float high, bool *fresh) {
  auto const key = std::make_pair(low, high);
  auto it = b->n0slot_of.find(key);
  *fresh = it == b->n0slot_of.end();
  int slot;
  if (!*fresh) {
    slot = it->second;
  } else {
    slot = (int)(std::find(b->n0slot_refs.begin(), b->n0slot_refs.end(), 0) - b->n0slot_refs.begin());  // the lowest free one
    if ((size_t)slot == b->n0slot_refs.size()) {
      if (b->n0slot_refs.size() >= (size_t)b->cfg.max_channels) {
        kq_internal_set_error("compute_n0 mask slots exhausted (%zu sets for %u channels)", b->n0slot_refs.size(), b->cfg.max_channels);
        return -1;
      }
      b->n0slot_refs.push_back(0);
      b->n0slot_key.push_back(key);
    }
    b->n0slot_key[slot] = key;
    b->n0slot_of[key] = slot;
  }
  b->n0slot_refs[slot]++;
  return slot;
}
void release_n0slot(kq_bank *b, int slot) {
  if (slot < 0 || (size_t)slot >= b->n0slot_refs.size() || b->n0slot_refs[slot] <= 0) return;
  if (--b->n0slot_refs[slot] == 0) b->n0slot_of.erase(b->n0slot_key[slot]);
}

int upload_n0mask(kq_bank *b, int c) {
  if (!b->chd.n0lane) return 0;
  int const nsub = b->use64k ? 4 : 1;
  bool fresh = false;
  int const old = b->chans[c].n0slot;
  auto const key = std::make_pair(b->chans[c].cfg.low, b->chans[c].cfg.high);
  if (old >= 0 && (size_t)old < b->n0slot_refs.size() && b->n0slot_refs[old] > 0 && b->n0slot_key[old] == key) {
    // unchanged edges keep their slot (and its reference)
    return ctl_put(b, CTL_FILTER, b->chd.n0slot + c, &old, sizeof(int)) ? -1 : 0;
  }
  // the old set goes back FIRST: in a full bank of distinct edges it is the only free one (asking first ran
  // one set past the planes).  Reusing it in place is safe: the mask write below is queued behind the filter passes in
  // flight, and no other channel refers to a slot whose count reached zero
  release_n0slot(b, old);
  b->chans[c].n0slot = -1;
  int const slot = acquire_n0slot(b, key.first, key.second, &fresh);
  if (slot < 0) return -1;
  b->chans[c].n0slot = slot;
  std::vector<unsigned long long> m;
  std::vector<unsigned> meta;
  if (fresh) {
    build_n0mask(b, b->chans[c].cfg.low, b->chans[c].cfg.high, m, meta);
    if (ctl_put(b, CTL_FILTER, b->chd.n0lane + (size_t)slot * nsub * 256, m.data(), m.size() * sizeof(m[0]))) return -1;
    if (ctl_put(b, CTL_FILTER, b->chd.n0meta + (size_t)slot * nsub, meta.data(), meta.size() * sizeof(unsigned))) return -1;
  }
  if (ctl_put(b, CTL_FILTER, b->chd.n0slot + c, &slot, sizeof(int))) return -1;
  return 0;
}

int channel_flags(const kq_channel_config &k) {
  bool const linear = k.demod_type == KQ_LINEAR_DEMOD;
  return (k.flat ? kq::FLAG_FLAT : 0) | (k.isb && linear ? kq::FLAG_ISB : 0) | (k.channels == 2 && linear ? kq::FLAG_STEREO : 0) |
         (k.square && linear ? kq::FLAG_SQUARE : 0);
}
Derived derive(const kq::Geom &g, const kq_channel_config &k) {
  Derived d;
  d.mode = k.demod_type;
  d.flags = channel_flags(k);
  float const samptime = (float)g.D / (float)g.samprate;  // am.c:21, linear.c:29
  float const rec_db = k.recovery_rate * samptime;
  d.recovery = powf(10.f, (float)((double)rec_db / 20.));  // dB2voltage, dsp.h:38
  d.hangmax = (int)(k.hangtime / samptime);                  // am.c:29, linear.c:38
  d.fm_gain = (float)((k.headroom * M_1_PI * g.dsamprate) / fabsf(k.low - k.high));  // fm.c:86
  d.init_gain = (d.mode == KQ_AM_DEMOD) ? powf(10.f, (float)(80. / 20.)) : powf(10.f, (float)(100.0 / 20.));
  return d;
}

// Derived per-channel constants, as each demod thread computes them in its prologue
// fresh = false: a new demodulator thread on an existing channel (set_mode): what struct demod keeps (sig.n0,
// sig.foffset, sig.pdeviation) is left alone
int upload_channel(kq_bank *b, int c, bool fresh) {
  // nothing here touches the device or waits: the writes gather in the control queues and the next call applies them --
  // what the filter kernels read in front of its filter pass, what the demodulators read and carry in front of its
  // demodulators, each behind the calls in flight
  HostChan &h = b->chans[c];
  kq::Geom const &g = b->g;
  kq_channel_config const &k = h.cfg;
  Derived const dv = derive(g, k);
  float const nan = NAN;
  float2 const one = make_float2(1.f, 0.f);  // fm.c:26
  auto const D = [&](void *dst, const void *src, size_t n) { return ctl_put(b, CTL_DEMOD, dst, src, n); };
  auto const Z = [&](void *dst, size_t n) { return ctl_fill(b, CTL_DEMOD, dst, 0u, n); };

  if (ctl_put(b, CTL_FILTER, b->chd.fflags + c, &dv.flags, sizeof(int))) return -1;
  if (ctl_put(b, CTL_FILTER, b->chd.low + c, &k.low, sizeof(float))) return -1;
  if (ctl_put(b, CTL_FILTER, b->chd.high + c, &k.high, sizeof(float))) return -1;
  if (D(b->chd.mode + c, &dv.mode, sizeof(int)) || D(b->chd.flags + c, &dv.flags, sizeof(int)) ||
      D(b->chd.fm_gain + c, &dv.fm_gain, sizeof(float)) || D(b->chd.headroom + c, &k.headroom, sizeof(float)) ||
      D(b->chd.recovery + c, &dv.recovery, sizeof(float)) || D(b->chd.hangmax + c, &dv.hangmax, sizeof(int)) ||
      D(b->chd.gain + c, &dv.init_gain, sizeof(float)) || (fresh && D(b->chd.n0 + c, &nan, sizeof(float))) ||
      D(b->chd.fm_state + c, &one, sizeof(float2)))
    return -1;
  // thread-local state of the demodulators at their prologue values (fm.c:26,68-69; am.c:26,33; linear.c:33)
  if (Z(b->chd.lastaudio + c, sizeof(float)) || Z(b->chd.sq_count + c, sizeof(int)) || Z(b->chd.hang + c, sizeof(int)) ||
      Z(b->chd.dc + c, sizeof(float)))
    return -1;
  if (g.Mdec > 1) {
    if (Z(b->chd.ahist + (size_t)c * (g.Mdec - 1), sizeof(float) * (g.Mdec - 1))) return -1;
    for (int kk = 0; kk < 2; kk++)
      if (b->fm_hist[kk] && Z(b->fm_hist[kk] + (size_t)c * (g.Mdec - 1), sizeof(float) * (g.Mdec - 1))) return -1;
  }
  if (fresh && (Z(b->chd.foffset + c, sizeof(float)) || Z(b->chd.pdev + c, sizeof(float)))) return -1;
  if (g.pl_n > 0) {
    if (Z(b->chd.plring + (size_t)c * 16384, sizeof(float) * 16384) || Z(b->chd.pl_ptr + c, sizeof(*b->chd.pl_ptr)) ||
        Z(b->chd.pl_last + c, sizeof(*b->chd.pl_last)))
      return -1;
  }
  if (D(b->chd.plfreq + c, &nan, sizeof(float))) return -1;
  if (upload_n0mask(b, c)) return -1;
  return 0;
}

// a channel's filter edges normalised to the output rate, as set_filter takes them (fm.c:35: low/dsamprate; am.c:41,
// linear.c:81: samptime*low).  `runtime`: a change made while running goes through display.c:161-177, which scales by
// samptime whatever the mode
void design_edges(const kq::Geom &g, const kq_channel_config &k, bool runtime, float *lo_n, float *hi_n) {
  if (k.demod_type == KQ_FM_DEMOD && !runtime) {
    *lo_n = k.low / g.dsamprate;
    *hi_n = k.high / g.dsamprate;
  } else {
    float const samptime = (float)g.D / (float)g.samprate;
    *lo_n = samptime * k.low;
    *hi_n = samptime * k.high;
  }
}

// Pre-detection response: set_filter with the channel's edges (design_edges).
// The design is queued for the next call's design launch (kq_bank::DesignQueue); the FM audio response (designed once, in
// the demodulator's prologue, fm.c:54-66) comes from the bank's cache by Kaiser beta -- designed, and waited for, the
// first time a beta is seen.
int queue_design(kq_bank *b, int c, bool runtime) {
  HostChan &h = b->chans[c];
  kq::Geom const &g = b->g;
  kq_bank::DesignQueue &d = b->dq;
  if (g.Ndec > 16384) {
    kq_internal_set_error("response design: N / decimate = %d exceeds 16384", g.Ndec);
    return -1;
  }
  float lo_n, hi_n;
  design_edges(g, h.cfg, runtime, &lo_n, &hi_n);
  if (!runtime) {
    if (h.cfg.demod_type == KQ_FM_DEMOD && !h.cfg.flat) {
      if (std::isnan(h.cfg.kaiser_beta)) {  // (not a key an ordered map can hold; the design takes it as the reference's does)
        h.aresp = kq::design_fm_audio_response(g.olen, g.Mdec, g.dsamprate, h.cfg.kaiser_beta);
        if (h.aresp.empty()) return -1;
      } else {
        auto it = b->aresp_cache.find(h.cfg.kaiser_beta);
        if (it == b->aresp_cache.end()) {
          std::vector<kq::cfloat> a = kq::design_fm_audio_response(g.olen, g.Mdec, g.dsamprate, h.cfg.kaiser_beta);
          if (a.empty()) return -1;
          if (b->aresp_cache.size() >= 64) b->aresp_cache.clear();
          it = b->aresp_cache.emplace(h.cfg.kaiser_beta, std::move(a)).first;
        }
        h.aresp = it->second;
      }
      if (ctl_put(b, CTL_DEMOD, b->chd.aresp + (size_t)c * (g.Ndec / 2 + 1), h.aresp.data(), sizeof(float2) * (g.Ndec / 2 + 1)))
        return -1;
    } else {
      h.aresp.clear();
    }
  }
  auto at = d.at.find(c);
  if (at == d.at.end() && d.jobs.size() >= d.max_jobs && ctl_flush_now(b)) return -1;  // (applies what has gathered, early)
  int const p = (int)(d.epoch & 1);
  float gain, ng_scale;
  kq::design_scales(g.N, h.out_type, &gain, &ng_scale);
  float2 *const row = b->chd.resp + (size_t)c * g.Ndec;
  float *const ng = d.ng_next + (size_t)p * b->cfg.max_channels + c;
  kq::DesignJob const job{lo_n, hi_n, h.cfg.kaiser_beta, gain};
  kq::DesignTarget const target{row, ng, ng_scale, 0.f};
  at = d.at.find(c);
  if (at != d.at.end()) {
    d.jobs[at->second] = job;
    d.targets[at->second] = target;
  } else {
    d.at[c] = (unsigned)d.jobs.size();
    d.jobs.push_back(job);
    d.targets.push_back(target);
  }
  ctl_cancel(b, CTL_FILTER, row);  // a response queued from the host for this row: the design runs in front of the queue
  h.resp.clear();                  // the host's copy: fetched when asked for
  return ctl_copy_dev(b, CTL_DEMOD, b->chd.noise_gain + c, ng, sizeof(float));
}
// the host's copy of a channel's response
int fetch_response(kq_bank *b, int c) {
  HostChan &h = b->chans[c];
  if (!h.resp.empty()) return 0;
  if (ctl_flush_now(b) || sync_all(b)) return -1;
  h.resp.resize(b->g.Ndec);
  KQ_TRY(hipMemcpy((void *)h.resp.data(), b->chd.resp + (size_t)c * b->g.Ndec, sizeof(float2) * b->g.Ndec, hipMemcpyDeviceToHost));
  return 0;
}

static int list_kind(const HostChan &h) {
  int const m = h.cfg.demod_type;
  if (m == KQ_LINEAR_DEMOD && h.cfg.pll) return 3;
  return m == KQ_FM_DEMOD ? 0 : m == KQ_AM_DEMOD ? 1 : 2;
}
// the lists from scratch (set-up, batched adds, anything that touches the carrier-loop list): ascending channel order
int upload_lists(kq_bank *b) {
  for (int k = 0; k < 3; k++) b->list_host[k].clear();
  b->list_pll_host.clear();
  b->list_active_host.clear();
  for (size_t c = 0; c < b->chans.size(); c++) {
    HostChan &h = b->chans[c];
    h.lk = h.lpos = h.apos = -1;
    if (!h.active) continue;
    h.apos = (int)b->list_active_host.size();
    b->list_active_host.push_back((int)c);
    h.lk = list_kind(h);
    std::vector<int> &l = h.lk == 3 ? b->list_pll_host : b->list_host[h.lk];  // (carrier loops: slot = position = order of creation)
    h.lpos = (int)l.size();
    l.push_back((int)c);
  }
  // the filter launch's list on the filter side; the demodulators' lists, and the PCM stage's copy of the active list,
  // on the demodulator side (the last call's demodulators may still be walking the old ones)
  size_t const n = b->list_active_host.size() * sizeof(int);
  {  // single entries queued while the lists were current (lists_add / lists_remove) give way to the rebuild
    size_t const whole = (size_t)b->cfg.max_channels * sizeof(int);
    ctl_cancel_range(b, CTL_FILTER, b->list_active_dev, whole);
    ctl_cancel_range(b, CTL_DEMOD, b->list_active_ds_dev, whole);
    if (b->list_pll_dev) ctl_cancel_range(b, CTL_DEMOD, b->list_pll_dev, whole);
    for (int k = 0; k < 3; k++) ctl_cancel_range(b, CTL_DEMOD, b->list_dev[k], whole);
  }
  if (ctl_put(b, CTL_FILTER, b->list_active_dev, b->list_active_host.data(), n)) return -1;
  if (ctl_put(b, CTL_DEMOD, b->list_active_ds_dev, b->list_active_host.data(), n)) return -1;
  if (!b->list_pll_host.empty())
    if (ctl_put(b, CTL_DEMOD, b->list_pll_dev, b->list_pll_host.data(), b->list_pll_host.size() * sizeof(int))) return -1;
  for (int k = 0; k < 3; k++)
    if (!b->list_host[k].empty())
      if (ctl_put(b, CTL_DEMOD, b->list_dev[k], b->list_host[k].data(), b->list_host[k].size() * sizeof(int))) return -1;
  b->lists_dirty = false;
  return 0;
}
// one channel onto / off the lists as they stand (nothing to do while a rebuild is pending; a carrier-loop channel asks for one)
int lists_add(kq_bank *b, int c) {
  if (b->lists_dirty) return 0;
  HostChan &h = b->chans[c];
  int const k = list_kind(h);
  if (k == 3) {
    b->lists_dirty = true;
    return 0;
  }
  h.apos = (int)b->list_active_host.size();
  b->list_active_host.push_back(c);
  if (ctl_put(b, CTL_FILTER, b->list_active_dev + h.apos, &c, sizeof(int))) return -1;
  if (ctl_put(b, CTL_DEMOD, b->list_active_ds_dev + h.apos, &c, sizeof(int))) return -1;
  h.lk = k;
  h.lpos = (int)b->list_host[k].size();
  b->list_host[k].push_back(c);
  return ctl_put(b, CTL_DEMOD, b->list_dev[k] + h.lpos, &c, sizeof(int));
}
// after a mode change: onto the new mode's list if that is another one
int lists_retype(kq_bank *b, int c) {
  if (b->lists_dirty) return 0;
  HostChan &h = b->chans[c];
  int const k = list_kind(h);
  if (k == 3 || h.lk == 3 || h.lk < 0) {
    b->lists_dirty = true;
    return 0;
  }
  if (k == h.lk) return 0;
  if (lists_remove(b, c, false)) return -1;
  h.lk = k;
  h.lpos = (int)b->list_host[k].size();
  b->list_host[k].push_back(c);
  return ctl_put(b, CTL_DEMOD, b->list_dev[k] + h.lpos, &c, sizeof(int));
}
int lists_remove(kq_bank *b, int c, bool from_active) {
  if (b->lists_dirty) return 0;
  HostChan &h = b->chans[c];
  if (h.lk == 3 || h.lk < 0 || h.lpos < 0 || h.apos < 0) {
    b->lists_dirty = true;
    return 0;
  }
  {
    std::vector<int> &l = b->list_host[h.lk];
    int const last = l.back();
    l[h.lpos] = last;
    b->chans[last].lpos = h.lpos;
    l.pop_back();
    if (last != c && ctl_put(b, CTL_DEMOD, b->list_dev[h.lk] + h.lpos, &last, sizeof(int))) return -1;
  }
  if (from_active) {
    std::vector<int> &l = b->list_active_host;
    int const last = l.back();
    l[h.apos] = last;
    b->chans[last].apos = h.apos;
    l.pop_back();
    if (last != c) {
      if (ctl_put(b, CTL_FILTER, b->list_active_dev + h.apos, &last, sizeof(int))) return -1;
      if (ctl_put(b, CTL_DEMOD, b->list_active_ds_dev + h.apos, &last, sizeof(int))) return -1;
    }
    h.apos = -1;
  }
  h.lk = h.lpos = -1;
  return 0;
}

}  // namespace kq::bank
