// kq_slots.hpp -- the host half that the slot banks share (kq_wfm, kq_rds, kq_rsmp and the PCM decoders below: up to
// max_slots decoders, each on a source row of the call's input, set and removed one at a time, processed together).  On
// top of kq::HostSide (kq_host.hpp); host only, so that it also compiles against the device-less stand-in for the runtime.
// The kernels, their argument blocks and the launches stay with each bank.
//
//   every slot bank   the slot table and its device copy, the staging of a host-memory call's distinct source rows, the
//                     copy-back of the active slots' rows, destroy / sync / remove, the argument checks of set and process
//   PCM decoders      (kq_fsk, kq_pag, kq_tone, kq_cw, kq_rtty, kq_psk, kq_acars, kq_ale, kq_dsc) the call's input binding
//                     (PcmIn, bind_pcm), the checks of a call and what is left of it (call_args_ok, begin_call), where the
//                     status records go and the tail of a host-memory call (bind_status, end_host_call), the checks the
//                     configs share (field_in_range, ...)
//   event banks       kq::EventArena: the [S][max_events] records and [S] counts.  kq_tone, kq_cw, kq_rtty, kq_psk, kq_ale
//                     and kq_dsc file events in it and take the bodies of pull_counts, pull_event and clear; kq_fsk, kq_pag
//                     and kq_acars keep their frame, page and block infos in one, take the counts and clear bodies, and
//                     pull a record with pull_record before they fetch its bytes themselves
//   deferred banks    (kq_cw, kq_rtty, kq_psk, kq_acars, kq_ale, kq_dsc) kq::DeferredSlots: set and remove touch no device;
//                     the next entry point that needs the device brings the changed slots there, a run at a time (flush)
//   frame-grid banks  (kq_cw, kq_rtty, kq_psk, kq_ale, kq_dsc) stand on kq_gridbank.hpp, on top of this file: one bank
//                     template and one body for create's tail, set's shared checks, process and the getters' opening
//
// A bank here is a struct on kq::HostSide with `cfg` (device, max_slots, max_samples), `mu`, `dev_ready`, `n_cur` (PCM
// decoders), `static constexpr bool kDeferred` (event banks) and the device half `d` that kq::lazy_device() makes, whose
// member `slots` is the bank's kq::SlotTable, `arena` its kq::EventArena and `st` the status plane of host-memory calls.  A
// deferred bank also has `def`, its kq::DeferredSlots, and `int to_device()`, which calls def.flush with the bank's own
// set-up and cold start.  `fn` is the entry point's name, for the error text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <optional>
#include <type_traits>
#include <vector>

#include "kq_device.hpp"
#include "kq_host.hpp"

namespace kq {

// where the kernels find a call's input: row r's block k begins at src + r src_stride + k row_stride (in samples); rowmap:
// per entry of the active list its row (a staged host-memory call), or null (the slot's own source row)
struct Staged {
  const void *src;
  size_t src_stride, row_stride;
  const int *rowmap;
};

// a call of PCM samples (KQ_PCM_F32 times `scale`, or KQ_PCM_S16BE) as the kernels' load_q reads it (kq_tonecorr.hpp):
// Staged's src and strides, the call's blocks block_len samples long
struct PcmIn {
  const void *src;
  int format;
  float scale;  // (where padding would be: the kernels' argument blocks are laid out as without it)
  size_t src_stride, row_stride;
  unsigned block_len;
};

// Par: the bank's per-slot record as the kernels read it, with `int active` and `unsigned source`
template <class Par>
struct SlotTable {
  std::vector<Par> par;     // [S]; empty until alloc()
  std::vector<int> all;     // active slots, ascending
  std::vector<int> rowmap;  // a host-memory call's: per entry of `all`, the staged row of its source
  Par *d_par = nullptr;
  int *d_list = nullptr, *d_rowmap = nullptr;
  char *d_stage = nullptr;  // host-memory calls: the distinct source rows, contiguous
  size_t stage_cap = 0;     // bytes

  bool active(unsigned slot) const { return slot < par.size() && par[slot].active; }

  int alloc(HostSide &h, size_t S) {
    par.assign(S, Par{});
    return h.alloc(&d_par, S, true) || h.alloc(&d_list, S) || h.alloc(&d_rowmap, S) ? -1 : 0;
  }

  // par[slot] and the active list to the device; waits, so the host copies may change again
  int upload(HostSide &h, unsigned slot) {
    KQ_TRY(hipMemcpyAsync(d_par + slot, &par[slot], sizeof(Par), hipMemcpyHostToDevice, h.stream));
    all.clear();
    for (size_t k = 0; k < par.size(); k++)
      if (par[k].active) all.push_back((int)k);
    if (!all.empty()) KQ_TRY(hipMemcpyAsync(d_list, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, h.stream));
    KQ_TRY(hipStreamSynchronize(h.stream));
    return 0;
  }

  // A host-memory call's input (samples of esize bytes, laid out as Staged says) to the device: the distinct source rows of
  // the active slots, numbered as they first appear along `all`, each with its blocks end to end.  The stage holds
  // cap_bytes_per_row for each.  (grow waits for the stream, which is idle here: the last host-memory call ended in a
  // synchronise, so it returns at once)
  int stage_rows(HostSide &h, const void *src, size_t esize, size_t src_stride, size_t row_stride, unsigned block_len,
                 unsigned nblocks, size_t cap_bytes_per_row, Staged *out) {
    return stage_rows(h, src, esize, src_stride, row_stride, block_len, nblocks, cap_bytes_per_row, out, 1u,
                      [](Par const &) { return 1u; });
  }

  // The same where a slot reads width(par) <= wmax elements per sample (interleaved sides): a staged block is wmax block_len
  // elements apart from the next, and of each block of a row what its widest reader takes is copied, no more (the caller's
  // rows of narrow readers need not be longer than those read).
  template <class W>
  int stage_rows(HostSide &h, const void *src, size_t esize, size_t src_stride, size_t row_stride, unsigned block_len,
                 unsigned nblocks, size_t cap_bytes_per_row, Staged *out, unsigned wmax, W width) {
    size_t const ncall = (size_t)block_len * nblocks * wmax, blk = (size_t)block_len * wmax;
    std::map<unsigned, std::pair<int, unsigned>> rows;  // source -> (staged row, elements per sample)
    rowmap.resize(all.size());
    for (size_t i = 0; i < all.size(); i++) {
      Par const &p = par[all[i]];
      auto const it = rows.emplace(p.source, std::make_pair((int)rows.size(), 1u)).first;
      it->second.second = std::max(it->second.second, (unsigned)width(p));
      rowmap[i] = it->second.first;
    }
    if (h.grow(&d_stage, &stage_cap, rows.size() * cap_bytes_per_row)) return -1;
    for (auto const &kv : rows) {
      size_t const w = (size_t)block_len * kv.second.second * esize;
      KQ_TRY(hipMemcpy2DAsync(d_stage + (size_t)kv.second.first * ncall * esize, blk * esize,
                               static_cast<const char *>(src) + (size_t)kv.first * src_stride * esize,
                               nblocks > 1 ? row_stride * esize : w, w, nblocks, hipMemcpyHostToDevice, h.stream));
    }
    KQ_TRY(hipMemcpyAsync(d_rowmap, rowmap.data(), rowmap.size() * sizeof(int), hipMemcpyHostToDevice, h.stream));
    *out = Staged{d_stage, ncall, blk, d_rowmap};
    return 0;
  }

  // f(first slot, count) for every maximal run of consecutive active slots; stops at the first f that does not return 0
  template <class F>
  int for_runs(F f) const {
    for (size_t i = 0; i < all.size();) {
      size_t j = i + 1;
      while (j < all.size() && all[j] == all[j - 1] + 1) j++;
      if (f((size_t)all[i], j - i)) return -1;
      i = j;
    }
    return 0;
  }
};

// the first `width` elements of rows first .. first + count - 1 of a device plane to the same rows of a host plane (strides
// in elements of elem_size bytes), queued on the handle's stream
inline int copy_rows_back(HostSide &h, void *dst, size_t dst_stride, const void *dev, size_t dev_stride, size_t width,
                          size_t elem_size, size_t first, size_t count) {
  KQ_TRY(hipMemcpy2DAsync(static_cast<char *>(dst) + first * dst_stride * elem_size, dst_stride * elem_size,
                           static_cast<const char *>(dev) + first * dev_stride * elem_size, dev_stride * elem_size,
                           width * elem_size, count, hipMemcpyDeviceToHost, h.stream));
  return 0;
}

// ---- entry points ---------------------------------------------------------------------------------------------------
template <class Bank>
int destroy_bank(Bank *b, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (b->dev_ready) {  // (otherwise the handle holds nothing: lazy_device)
    DeviceScope dev_scope_(b->cfg.device);
    b->close();
  }
  delete b;
  return 0;
}

template <class Bank>
int sync_bank(Bank *b, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

template <class Bank>
int remove_slot(Bank *b, unsigned slot, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  auto &t = b->d.slots;
  if (!t.active(slot)) {
    kq_internal_set_error("%s: slot %u holds no decoder", fn, slot);
    return -1;
  }
  DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  t.par[slot] = {};
  return t.upload(*b, slot);
}

// kq_*_reset of a PCM decoder bank whose set touches the device: the stream index back to 0, cold(slot) -> 0 / -1 queued for
// every active slot, between two waits
template <class Bank, class Cold>
int reset_slots(Bank *b, const char *fn, Cold cold) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  if (!b->dev_ready) return 0;
  DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  for (int s : b->d.slots.all)
    if (cold((unsigned)s)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// kq_*_set before it has looked at the bank: the slot against any bank's limit, the parameters there at all
inline bool set_args_ok(const char *fn, unsigned slot, const void *params, unsigned slot_limit) {
  if (slot >= slot_limit) {
    kq_internal_set_error("%s: slot %u is beyond any bank (%u slots at most)", fn, slot, slot_limit);
    return false;
  }
  if (!params) kq_internal_set_error("%s: null params", fn);
  return params != nullptr;
}

// ... and the slot against this bank's
inline bool slot_in_bank(const char *fn, unsigned slot, unsigned max_slots) {
  if (slot >= max_slots) kq_internal_set_error("%s: slot %u >= max_slots %u", fn, slot, max_slots);
  return slot < max_slots;
}

// kq_*_process: the call's blocks against the bank's max_samples and the rows they lie in
inline bool blocks_ok(const char *fn, size_t max_samples, size_t row_stride, unsigned block_len, unsigned nblocks) {
  size_t const ncall = (size_t)block_len * nblocks;
  if (ncall > max_samples) {
    kq_internal_set_error("%s: nblocks %u x block_len %u = %zu > max_samples %zu", fn, nblocks, block_len, ncall, max_samples);
    return false;
  }
  if (nblocks > 1 && row_stride < block_len) {
    kq_internal_set_error("%s: row_stride %zu < block_len %u", fn, row_stride, block_len);
    return false;
  }
  return true;
}

// kq_*_process, once the bank's own checks of the output strides have passed: what is left of the call
enum CallWork {
  CALL_FAILED = -1,  // null source (`src_name`: the parameter's name); the error text is set
  CALL_EMPTY = 0,    // no samples: nothing happens
  CALL_IDLE,         // no active slot: only the stream index moves
  CALL_RUN
};
template <class Bank>
CallWork call_work(const Bank *b, const char *fn, size_t ncall, const void *src, const char *src_name) {
  if (ncall == 0) return CALL_EMPTY;
  if (!src) {
    kq_internal_set_error("%s: null %s", fn, src_name);
    return CALL_FAILED;
  }
  return b->d.slots.all.empty() || !b->dev_ready ? CALL_IDLE : CALL_RUN;
}

// ---- kq_*_create: the checks that the configs of the PCM decoders share ------------------------------------------------
// Each bank calls them in the order it reports them, with its own limits.
inline bool field_in_range(const char *fn, const char *name, unsigned v, unsigned lo, unsigned hi) {
  if (v < lo || v > hi) kq_internal_set_error("%s: %s %u must be %u..%u", fn, name, v, lo, hi);
  return v >= lo && v <= hi;
}

inline bool samprate_ok(const char *fn, double Fs) {
  bool const ok = Fs > 0 && std::isfinite(Fs);
  if (!ok) kq_internal_set_error("%s: samprate %.10g must be positive and finite", fn, Fs);
  return ok;
}

inline bool min_p_ok(const char *fn, unsigned long long min_p) {
  if (min_p > (1ull << 55)) kq_internal_set_error("%s: min_p %llu must be 0..2^55", fn, min_p);
  return min_p <= (1ull << 55);
}

inline bool input_scale_ok(const char *fn, float scale) {
  bool const ok = std::isfinite(scale) && scale > 0;
  if (!ok) kq_internal_set_error("%s: input_scale must be finite and positive", fn);
  return ok;
}

inline bool max_samples_ok(const char *fn, size_t max_samples) {
  bool const ok = max_samples != 0 && max_samples <= ((size_t)1 << 28);
  if (!ok) kq_internal_set_error("%s: max_samples %zu must be 1..2^28", fn, max_samples);
  return ok;
}

// ---- kq_*_process of the PCM decoders: the call's checks, its input, its status records and its tail -------------------
// the sample format, the blocks (blocks_ok) and the status stride, in the order the entry points report them
inline bool call_args_ok(const char *fn, int format, size_t max_samples, size_t row_stride, unsigned block_len, unsigned nblocks,
                         const void *status, size_t status_stride) {
  if (format != KQ_PCM_F32 && format != KQ_PCM_S16BE) {
    kq_internal_set_error("%s: unknown sample format %d", fn, format);
    return false;
  }
  if (!blocks_ok(fn, max_samples, row_stride, block_len, nblocks)) return false;
  if (status && status_stride < 1) kq_internal_set_error("%s: status_stride %zu < 1", fn, status_stride);
  return !status || status_stride >= 1;
}

// The call's input as the kernels find it: the caller's device pointer (*rowmap null: a slot reads its own source row), or a
// host-memory call's distinct rows staged (the stage holds 4 bytes per sample whatever the format; the rows lie as closely
// as the format allows) and *rowmap, per entry of the active list, its row there.
template <class Par>
int bind_pcm(PcmIn *in, const int **rowmap, HostSide &h, SlotTable<Par> &slots, size_t max_samples, float scale, const void *src, int format,
             size_t src_stride, size_t row_stride, unsigned block_len, unsigned nblocks, int on_device) {
  in->src = src;
  in->format = format;
  in->scale = scale;
  in->src_stride = src_stride;
  in->row_stride = row_stride;
  in->block_len = block_len;
  *rowmap = nullptr;
  if (on_device) return 0;
  Staged st;
  if (slots.stage_rows(h, src, format == KQ_PCM_S16BE ? 2 : 4, src_stride, row_stride, block_len, nblocks, max_samples * 4, &st))
    return -1;
  in->src = st.src;
  in->src_stride = st.src_stride;
  in->row_stride = st.row_stride;
  *rowmap = st.rowmap;
  return 0;
}

// What an entry point that reads the device does first, the bank's lock held.  1: the bank has no device and needs none,
// the answer is "nothing"; 0: `scope` holds the bank's device, and a deferred bank's changed slots are there; -1: failed.
template <class Bank>
int device_for_read(Bank *b, std::optional<DeviceScope> &scope) {
  if constexpr (Bank::kDeferred) {
    if (b->def.deviceless(b->dev_ready)) {
      (void)b->to_device();  // forgets the changes: there is nowhere to bring them
      return 1;
    }
    scope.emplace(b->cfg.device);
    return b->to_device() ? -1 : 0;
  } else {
    if (!b->dev_ready) return 1;
    scope.emplace(b->cfg.device);
    return 0;
  }
}

// call_work for these banks, after call_args_ok and the bank's own checks: an idle call moves the stream index here, and
// CALL_RUN leaves the bank's device in `scope`
template <class Bank>
CallWork begin_call(Bank *b, const char *fn, size_t ncall, const void *src, std::optional<DeviceScope> &scope) {
  if (ncall == 0) return CALL_EMPTY;
  if (!src) {
    kq_internal_set_error("%s: null src", fn);
    return CALL_FAILED;
  }
  int const r = device_for_read(b, scope);
  if (r < 0) return CALL_FAILED;
  if (r == 0 && !b->d.slots.all.empty()) return CALL_RUN;
  b->n_cur += ncall;
  return CALL_IDLE;
}

// where the kernel writes the status records: the caller's device plane, or for a host-memory call the bank's own d.st
// (made when first asked for) at stride 1
template <class Bank, class St>
int bind_status(Bank *b, int on_device, St *status, size_t status_stride, St **st, size_t *sstride) {
  if (!on_device && status && !b->d.st && b->alloc(&b->d.st, (size_t)b->cfg.max_slots)) return -1;
  *st = on_device || !status ? status : b->d.st;
  *sstride = on_device ? status_stride : 1;
  return 0;
}

// the tail of a host-memory call, behind the launch: the records of the active slots to the caller's plane, with whatever
// else the bank copies back per run of slots (`more`: null, or (first, count) -> 0 / -1), and the wait
template <class Bank, class St, class More>
int end_host_call(Bank *b, St *status, size_t status_stride, More more) {
  auto back = [&](size_t s0, size_t n) {
    if (status && copy_rows_back(*b, status, status_stride, b->d.st, 1, 1, sizeof(St), s0, n)) return -1;
    if constexpr (!std::is_same<More, std::nullptr_t>::value) return more(s0, n);
    return 0;
  };
  if ((status || !std::is_same<More, std::nullptr_t>::value) && b->d.slots.for_runs(back)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// ---- event banks -----------------------------------------------------------------------------------------------------
// Per slot an arena of up to `cap` records that the kernel files in order, and how many it holds.
template <class Event>
struct EventArena {
  Event *ev = nullptr;    // [S][cap]
  unsigned *n = nullptr;  // [S]
  size_t cap = 0;

  int alloc(HostSide &h, size_t S, size_t max_events) {
    cap = max_events;
    return h.alloc(&ev, S * max_events) || h.alloc(&n, S, true) ? -1 : 0;
  }

  // the arenas of `count` slots from `first` are empty (queued on the handle's stream)
  int clear(HostSide &h, size_t first, size_t count) {
    KQ_TRY(hipMemsetAsync(n + first, 0, count * sizeof(unsigned), h.stream));
    return 0;
  }
};

template <class Bank>
int pull_counts(Bank *b, const char *fn, uint32_t *counts) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!counts) {
    kq_internal_set_error("%s: null counts", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  std::optional<DeviceScope> scope;
  int const r = device_for_read(b, scope);  // (a deferred slot set since the last call shows its empty arena)
  if (r == 1) std::memset(counts, 0, b->cfg.max_slots * sizeof(uint32_t));
  if (r) return r < 0 ? -1 : 0;
  KQ_TRY(hipMemcpyAsync(counts, b->d.arena.n, b->cfg.max_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// record `index` of `slot`'s arena to *rec, the bank's lock held; `what`: the records' name in the error text.  *at: where
// it lies in the arena, for the banks that keep more per record than the arena holds
template <class Bank, class Event>
int pull_record(Bank *b, const char *fn, unsigned slot, unsigned index, const char *what, Event *rec, size_t *at,
                std::optional<DeviceScope> &scope) {
  if (slot >= b->cfg.max_slots) {
    kq_internal_set_error("%s: slot %u >= max_slots %u", fn, slot, b->cfg.max_slots);
    return -1;
  }
  unsigned n = 0;
  int const r = device_for_read(b, scope);
  if (r < 0) return -1;
  if (r == 0) {
    KQ_TRY(hipMemcpyAsync(&n, b->d.arena.n + slot, sizeof n, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (index >= n) {
    kq_internal_set_error("%s: slot %u has %u %s", fn, slot, n, what);
    return -1;
  }
  *at = (size_t)slot * b->d.arena.cap + index;
  KQ_TRY(hipMemcpyAsync(rec, b->d.arena.ev + *at, sizeof *rec, hipMemcpyDeviceToHost, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

template <class Bank, class Event>
int pull_event(Bank *b, const char *fn, unsigned slot, unsigned index, Event *event) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!event) {
    kq_internal_set_error("%s: null event", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  std::optional<DeviceScope> scope;
  size_t at;
  return pull_record(b, fn, slot, index, "events", event, &at, scope);
}

template <class Bank>
int clear_arena(Bank *b, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  DeviceScope dev_scope_(b->cfg.device);
  return b->d.arena.clear(*b, 0, b->cfg.max_slots);
}

// ---- deferred banks --------------------------------------------------------------------------------------------------
// set and remove touch no device: they change `want`, and the next entry point that needs the device brings the slots in
// `dirty` there (flush), a cold start for each that is set.
template <class Par>
struct DeferredSlots {
  std::vector<Par> want;        // [S]
  std::vector<unsigned> dirty;  // the slots set or removed since the last flush, each once
  std::vector<char> is_dirty;   // [S]
  size_t nwant = 0;             // active entries of `want`

  void init(size_t S) {
    want.assign(S, Par{});
    is_dirty.assign(S, 0);
  }

  // no device yet and no slot that wants one: the entry points then ask for none
  bool deviceless(bool dev_ready) const { return !dev_ready && nwant == 0; }
  bool is_set(unsigned slot) const { return slot < want.size() && want[slot].active; }

  void touch(unsigned slot) {
    if (is_dirty[slot]) return;
    is_dirty[slot] = 1;
    dirty.push_back(slot);
  }

  // the tail of kq_*_set, once the bank has made the slot's record
  void set(unsigned slot, Par const &p) {
    nwant += !want[slot].active;
    want[slot] = p;
    touch(slot);
  }

  // The slots that were set or removed since the last call, to the device `make` makes where there is none yet
  // (kq::lazy_device).  cold(first, count) queues the cold start of a run of slots that are set: their carried state as
  // the header has it at the set, their arenas empty; what it copies from must live until flush returns.  Consecutive slots
  // go together: a run costs one copy of its parameters and one cold(), however long it is (4096 slots set before the first
  // call are a handful of runtime calls, not thousands).  Waits for the stream first and last.  Without a device and without
  // a slot that wants one the changes are forgotten.
  template <class Bank, class Make, class Cold>
  int flush(Bank *b, Make make, Cold cold) {
    if (dirty.empty()) return 0;
    auto forget = [this] {
      for (unsigned s : dirty) is_dirty[s] = 0;
      dirty.clear();
    };
    if (deviceless(b->dev_ready)) {
      forget();
      return 0;
    }
    if (lazy_device(b, make)) return -1;
    KQ_TRY(hipStreamSynchronize(b->stream));
    auto &t = b->d.slots;
    std::sort(dirty.begin(), dirty.end());
    for (unsigned s : dirty) t.par[s] = want[s];
    for (size_t i = 0; i < dirty.size();) {  // a run: consecutive slots, all set or all removed
      unsigned const s0 = dirty[i];
      int const set = t.par[s0].active;
      size_t j = i + 1;
      while (j < dirty.size() && dirty[j] == dirty[j - 1] + 1 && t.par[dirty[j]].active == set) j++;
      if (set && cold((size_t)s0, j - i)) return -1;
      KQ_TRY(hipMemcpyAsync(t.d_par + s0, &t.par[s0], (j - i) * sizeof(Par), hipMemcpyHostToDevice, b->stream));  // (t.par stays)
      i = j;
    }
    if (t.upload(*b, dirty.back())) return -1;  // the active list and the wait (and that one record once more)
    forget();
    return 0;
  }
};

template <class Bank>
int deferred_remove(Bank *b, unsigned slot, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->def.is_set(slot)) {
    kq_internal_set_error("%s: slot %u holds no decoder", fn, slot);
    return -1;
  }
  b->def.want[slot] = {};
  b->def.nwant--;
  b->def.touch(slot);
  return 0;
}

// the stream index back to 0; every slot that is set starts cold at the next call
template <class Bank>
int deferred_reset(Bank *b, const char *fn) {
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  for (unsigned s = 0; s < b->def.want.size(); s++)
    if (b->def.want[s].active) b->def.touch(s);
  return 0;
}

}  // namespace kq
