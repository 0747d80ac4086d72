// kq_slots.hpp -- the host half that the slot banks share (kq_wfm, kq_rds, kq_fsk, kq_pag, kq_tone, kq_cw, kq_rtty, kq_rsmp: up to max_slots decoders, each on
// a source row of the call's input, set and removed one at a time, processed together): the slot table and its device copy, the
// staging of a host-memory call's distinct source rows, the copy-back of the active slots' rows, and the bodies of the entry
// points that do not differ from bank to bank.  On top of kq::HostSide (kq_host.hpp); host only.  The kernels, their
// argument blocks and the launches stay with each bank.
//
// A bank here is a struct on kq::HostSide with `cfg` (device, max_samples), `mu`, `dev_ready` and the device half `d` that
// kq::lazy_device() makes, whose member `slots` is the bank's kq::SlotTable.  `fn` is the entry point's name, for the error
// text.
#pragma once
#include <map>
#include <mutex>
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

}  // namespace kq
