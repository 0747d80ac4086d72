// kq_pag.hip -- POCSAG pager decoder bank: flat FM discriminator output -> pages (512, 1200 or 2400 bit/s direct FSK) on
// gfx950.
//
// Per slot (include/ka9q_hip.h, kq_pag_*): the front end of kq_fsk_* bit for bit (kq_fskfront.hpp: quantiser, low-pass,
// windowed mid-level threshold, shift DPLL), then batch synchronisation on the frame-sync codeword in either polarity,
// BCH(31,21) + parity correction of up to two bits per codeword by a table, and the assembly of pages.  All integer after
// the quantiser.  State on the device, per slot: the front end's, PagState (clock, deframer, the open page's record), the
// open page's words, the arena of closed pages; per bank the correction table.
//
// k_fsk_front  kq_fskfront.hpp, shared with kq_fsk
// k_pag_track  one lane per slot: the call's words in order through DPLL and deframer; pages and status out.  Serial by
//              nature, as k_fsk_track is; the open page lives in global memory, written three bytes at a time.  The
//              syndrome is 21 shift / xor steps in registers, once per 32 channel bits; the error pattern is one load from
//              the 8 KiB table
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_device.hpp"
#include "kq_fskfront.hpp"
#include "kq_host.hpp"
#include "kq_slots.hpp"

namespace {

using kq::fskfront::kMaxSlots;
using kq::fskfront::pll_step;
using PagGeom = kq::fskfront::Geom;

constexpr uint32_t kGen = 0x769u;               // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
constexpr uint32_t kNoFix = 0xFFFFFFFFu;        // the table's "uncorrectable" (no pattern of weight <= 2)
constexpr int kFixEntries = 2048;

struct PagPar {  // per slot, written by the host at kq_pag_set
  int active;
  unsigned source;
};

struct PagState {  // per slot, carried from call to call; all zero when a slot is set
  int s, dprev;                  // the bit clock
  unsigned sh;
  int synced, inv, cnt, pos, miss;
  int open;                      // a page is open: its record so far
  unsigned ric, function, nwords, flags, errors;
  unsigned long long end_sample;
  unsigned bits, syncs, batches, sync_missed, words_good, words_fixed, words_bad, orphans, pages, dropped;
};

struct CallArgs {
  kq::fskfront::FrontArgs<PagPar> f;   // the front end's; k_pag_track reads its geometry, list, dw, level, n0, n1, w0
  int max_pages, mpw;
  const uint32_t *fix;           // [2048]: (syndrome << 1 | parity) -> error pattern, or kNoFix
  PagState *state;               // [S]
  unsigned char *open;           // [S][3 mpw]
  unsigned char *pages;          // [S][max_pages][3 mpw]
  kq_pag_page_info *info;        // [S][max_pages]
  unsigned *npages;              // [S]
  // output
  kq_pag_status *st;
  size_t sstride;
};

// the remainder of bits 31..1 of x, as a polynomial of degree 30, by g: 21 steps
__host__ __device__ inline uint32_t syndrome(uint32_t x) {
  uint32_t r = x >> 1;
#pragma unroll
  for (int i = 30; i >= 10; i--)
    if ((r >> i) & 1u) r ^= kGen << (i - 10);
  return r & 0x3FFu;
}

__host__ __device__ inline int popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

__host__ __device__ inline unsigned fix_index(uint32_t x) { return (syndrome(x) << 1) | (unsigned)(popc(x) & 1); }

struct PageOut {
  unsigned char *open;
  unsigned char *pages;
  kq_pag_page_info *info;
  unsigned n;                    // pages in the arena
  int max_pages, mpw;
};

__device__ __forceinline__ void close_page(PagState &s, unsigned flag, PageOut &o) {
  s.flags |= flag;
  s.pages++;
  s.open = 0;
  if (o.n >= (unsigned)o.max_pages) {
    s.dropped++;
    return;
  }
  unsigned char *dst = o.pages + (size_t)o.n * 3 * o.mpw;
  for (unsigned i = 0; i < 3 * s.nwords; i++) dst[i] = o.open[i];
  kq_pag_page_info r;
  r.ric = s.ric;
  r.function = s.function;
  r.nwords = s.nwords;
  r.flags = s.flags;
  r.errors = s.errors;
  r.reserved = 0;
  r.end_sample = s.end_sample;
  o.info[o.n] = r;
  o.n++;
}

// a message word to the open page (the caller has seen that it has room)
__device__ __forceinline__ void append_word(PagState &s, uint32_t x, unsigned code, PageOut &o, int64_t n) {
  uint32_t const w = (code << 20) | ((x >> 11) & 0xFFFFFu);
  unsigned char *p = o.open + 3 * s.nwords;
  p[0] = (unsigned char)(w >> 16);
  p[1] = (unsigned char)(w >> 8);
  p[2] = (unsigned char)w;
  s.nwords++;
  s.end_sample = (unsigned long long)n;
}

// one channel bit through the deframer (the header's "hunting" .. "codeword position")
__device__ __forceinline__ void push_bit(PagState &s, unsigned c, const uint32_t *fix, PageOut &o, int64_t n) {
  s.sh = (s.sh << 1) | c;
  if (!s.synced) {
    bool const up = popc(s.sh ^ KQ_PAG_FSC) <= 2;
    if (up || popc(~s.sh ^ KQ_PAG_FSC) <= 2) {
      s.synced = 1;
      s.inv = up ? 0 : 1;
      s.cnt = s.pos = s.miss = 0;
      s.syncs++;
      s.batches++;
    }
    return;
  }
  if (++s.cnt < 32) return;
  s.cnt = 0;
  uint32_t const x = s.inv ? ~s.sh : s.sh;
  if (s.pos == 16) {
    s.pos = 0;
    if (popc(x ^ KQ_PAG_FSC) <= 2) {
      s.batches++;
      s.miss = 0;
      return;
    }
    s.sync_missed++;
    if (++s.miss == 2) {
      s.synced = 0;
      if (s.open) close_page(s, KQ_PAG_LOST, o);
    }
    return;
  }
  int const frame = s.pos >> 1;
  s.pos++;
  uint32_t const e = fix[fix_index(x)];
  if (e == kNoFix) {
    s.words_bad++;
    if (s.open && s.nwords < (unsigned)o.mpw) {
      append_word(s, x, 3u, o, n);
      s.flags |= KQ_PAG_BAD;
    }
    return;
  }
  uint32_t const v = x ^ e;
  unsigned const ne = (unsigned)popc(e);
  if (ne) s.words_fixed++;
  else s.words_good++;
  if (v == KQ_PAG_IDLE) {
    if (s.open) close_page(s, 0u, o);
  } else if (!(v >> 31)) {
    if (s.open) close_page(s, 0u, o);
    s.open = 1;
    s.ric = (((v >> 13) & 0x3FFFFu) << 3) | (unsigned)frame;
    s.function = (v >> 11) & 3u;
    s.nwords = 0;
    s.flags = 0;
    s.errors = ne;
    s.end_sample = (unsigned long long)n;
  } else if (!s.open) {
    s.orphans++;
  } else if (s.nwords < (unsigned)o.mpw) {
    append_word(s, v, ne, o, n);
    s.errors += ne;
  } else {
    close_page(s, KQ_PAG_FULL, o);
    s.orphans++;
  }
}

// one lane per slot: the call's samples in order
__global__ __launch_bounds__(64) void k_pag_track(CallArgs c, int nlist) {
  int const li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nlist) return;
  kq::fskfront::FrontArgs<PagPar> const &a = c.f;
  int const slot = a.list[li];
  PagGeom const &g = a.g;
  PagState s = c.state[slot];
  PageOut o;
  o.open = c.open + (size_t)slot * 3 * c.mpw;
  o.pages = c.pages + (size_t)slot * c.max_pages * 3 * c.mpw;
  o.info = c.info + (size_t)slot * c.max_pages;
  o.n = c.npages[slot];
  o.max_pages = c.max_pages;
  o.mpw = c.mpw;
  int64_t n = a.n0;
  while (n < a.n1) {
    int const b0 = (int)(n & 63);
    int64_t const left = a.n1 - n;
    int const cnt = (int)(left < 64 - b0 ? left : 64 - b0);
    unsigned long long word = a.dw[(size_t)((n >> 6) - a.w0) * g.S + slot] >> b0;
    for (int k = 0; k < cnt; k++, word >>= 1, n++) {
      int const d = (int)(word & 1u);
      if (!pll_step(s.s, s.dprev, d, g)) continue;
      s.bits++;
      push_bit(s, (unsigned)d, c.fix, o, n);
    }
  }
  c.state[slot] = s;
  c.npages[slot] = o.n;
  if (c.st) {
    kq_pag_status r;
    r.bits = s.bits;
    r.syncs = s.syncs;
    r.batches = s.batches;
    r.sync_missed = s.sync_missed;
    r.words_good = s.words_good;
    r.words_fixed = s.words_fixed;
    r.words_bad = s.words_bad;
    r.orphans = s.orphans;
    r.pages = s.pages;
    r.dropped = s.dropped;
    r.pll_phase = s.s;
    r.synced = s.synced;
    r.inverted = s.inv;
    r.level = a.level[slot];
    c.st[(size_t)slot * c.sstride] = r;
  }
}

// (syndrome, parity) -> the error pattern of weight <= 2 over the 32 bits, from the generator: 1 + 32 + 496 patterns, which
// the extended code's minimum distance of 6 keeps apart; every other entry kNoFix.  Built once: by the first kq_pag_create,
// or by kq_pag_correct where that comes first (it needs no bank).
std::vector<uint32_t> const &fix_table() {
  static std::vector<uint32_t> const table = [] {
    std::vector<uint32_t> t((size_t)kFixEntries, kNoFix);
    t[fix_index(0u)] = 0u;
    for (int i = 0; i < 32; i++) {
      t[fix_index(1u << i)] = 1u << i;
      for (int j = 0; j < i; j++) t[fix_index((1u << i) | (1u << j))] = (1u << i) | (1u << j);
    }
    return t;
  }();
  return table;
}

}  // namespace

struct kq_pag_bank : kq::HostSide {
  static constexpr bool kDeferred = false;
  kq_pag_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  PagGeom g{};
  int max_pages = 0, mpw = 0;
  uint64_t n_cur = 0;
  int turn = 0;                          // the copy of the carried q the next call reads
  std::vector<short> hq;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<PagPar> slots;
    kq::fskfront::FrontDev front;
    uint32_t *fix = nullptr;
    PagState *state = nullptr;
    unsigned char *open = nullptr, *pages = nullptr;
    kq::EventArena<kq_pag_page_info> arena;  // the pages' infos and how many there are
    kq_pag_status *st = nullptr;         // host-memory calls
  } d;
};

namespace {

int make_device(kq_pag_bank *b) {
  auto &d = b->d;
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_slots, mp = (size_t)b->max_pages, pb = 3 * (size_t)b->mpw;
  if (d.slots.alloc(*b, S) || d.front.alloc(*b, b->g, b->hq) || b->alloc(&d.fix, (size_t)kFixEntries) ||
      b->alloc(&d.state, S, true) || b->alloc(&d.open, S * pb, true) || b->alloc(&d.pages, S * mp * pb) ||
      d.arena.alloc(*b, S, mp))
    return -1;
  KQ_TRY(hipMemcpyAsync(d.fix, fix_table().data(), kFixEntries * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// zero history, clock, deframer and arena (the stream is idle: callers synchronised it)
int cold_start(kq_pag_bank *b, unsigned s) {
  if (b->d.front.cold_start(*b, b->g, s)) return -1;
  KQ_TRY(hipMemsetAsync(b->d.state + s, 0, sizeof(PagState), b->stream));
  return b->d.arena.clear(*b, s, 1);
}

}  // namespace

extern "C" {

int kq_pag_correct(uint32_t word, uint32_t *fixed) {
  uint32_t const e = fix_table()[fix_index(word)];
  if (e == kNoFix) return -1;
  if (fixed) *fixed = word ^ e;
  return popc(e);
}

kq_pag_bank *kq_pag_create(const kq_pag_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_pag_create: null config");
    return nullptr;
  }
  kq::fskfront::FrontConfig const fc{cfg->samprate,    cfg->baud,        cfg->taps,      cfg->cutoff_hz, cfg->kaiser_beta,
                                     cfg->window_bits, cfg->input_scale, cfg->pll_shift, cfg->max_slots, cfg->max_samples};
  PagGeom g{};
  std::vector<short> hq;
  if (!kq::fskfront::front_config("kq_pag_create", fc, &g, &hq)) return nullptr;
  if (!kq::field_in_range("kq_pag_create", "max_pages", cfg->max_pages, 1, 4096) ||
      !kq::field_in_range("kq_pag_create", "max_page_words", cfg->max_page_words, 1, 256))
    return nullptr;
  (void)fix_table();  // the correction table exists from here on
  kq_pag_bank *b = new kq_pag_bank;
  b->cfg = *cfg;
  b->hq = std::move(hq);
  b->g = g;
  b->max_pages = (int)cfg->max_pages;
  b->mpw = (int)cfg->max_page_words;
  return b;
}

int kq_pag_destroy(kq_pag_bank *b) { return kq::destroy_bank(b, "kq_pag_destroy"); }

int kq_pag_set(kq_pag_bank *b, unsigned slot, const kq_pag_params *p) {
  if (!kq::set_args_ok("kq_pag_set", slot, p, kMaxSlots)) return -1;
  if (!b) {
    kq_internal_set_error("kq_pag_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::slot_in_bank("kq_pag_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  PagPar np{};
  np.active = 1;
  np.source = p->source;
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_pag_remove(kq_pag_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_pag_remove"); }

int kq_pag_process(kq_pag_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_pag_status *status, size_t status_stride) {
  const char *fn = "kq_pag_process";
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!kq::call_args_ok(fn, format, b->cfg.max_samples, row_stride, block_len, nblocks, status, status_stride)) return -1;
  size_t const ncall = (size_t)block_len * nblocks;
  std::optional<kq::DeviceScope> scope;
  kq::CallWork const work = kq::begin_call(b, fn, ncall, src, scope);
  if (work != kq::CALL_RUN) return work == kq::CALL_FAILED ? -1 : 0;
  auto &d = b->d;
  size_t const nlist = d.slots.all.size();
  CallArgs a{};
  if (kq::fskfront::bind_front(&a.f, *b, d.slots, d.front, b->g, b->turn, b->n_cur, b->cfg.max_samples, src, format, src_stride,
                               row_stride, block_len, nblocks, on_device) ||
      kq::bind_status(b, on_device, status, status_stride, &a.st, &a.sstride))
    return -1;
  a.max_pages = b->max_pages;
  a.mpw = b->mpw;
  a.fix = d.fix;
  a.state = d.state;
  a.open = d.open;
  a.pages = d.pages;
  a.info = d.arena.ev;
  a.npages = d.arena.n;
  if (kq::fskfront::launch_front(a.f, nlist, b->stream)) return -1;
  hipLaunchKernelGGL(k_pag_track, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, b->stream, a, (int)nlist);
  KQ_TRY(hipGetLastError());
  b->turn ^= 1;  // from here on the carried q is in the other copy, whatever fails below
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_pag_pull_counts(kq_pag_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_pag_pull_counts", counts); }

int kq_pag_pull_page(kq_pag_bank *b, unsigned slot, unsigned index, unsigned char *dst, size_t cap, kq_pag_page_info *info) {
  const char *fn = "kq_pag_pull_page";
  if (!b) {
    kq_internal_set_error("%s: null bank", fn);
    return -1;
  }
  if (!dst) {
    kq_internal_set_error("%s: null dst", fn);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  std::optional<kq::DeviceScope> scope;
  kq_pag_page_info r;
  size_t at;
  if (kq::pull_record(b, fn, slot, index, "pages", &r, &at, scope)) return -1;
  size_t const take = std::min(cap, (size_t)3 * r.nwords);
  if (take) {
    KQ_TRY(hipMemcpyAsync(dst, b->d.pages + at * 3 * b->mpw, take, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (info) *info = r;
  return (int)(3 * r.nwords);
}

int kq_pag_clear_pages(kq_pag_bank *b) { return kq::clear_arena(b, "kq_pag_clear_pages"); }

int kq_pag_get_taps(const kq_pag_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_pag_get_taps: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_pag_get_taps: null dst");
    return -1;
  }
  size_t const n = std::min(cap, b->hq.size());
  if (n) std::memcpy(dst, b->hq.data(), n * sizeof(int16_t));
  return (int)b->hq.size();
}

int kq_pag_sync(kq_pag_bank *b) { return kq::sync_bank(b, "kq_pag_sync"); }

int kq_pag_reset(kq_pag_bank *b) {
  return kq::reset_slots(b, "kq_pag_reset", [b](unsigned s) { return cold_start(b, s); });
}

}  // extern "C"
