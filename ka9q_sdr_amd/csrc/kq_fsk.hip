// kq_fsk.hip -- baseband FSK / GMSK packet decoder bank: flat FM discriminator output -> HDLC frames (9600 bit/s G3RUH,
// AIS) on gfx950.
//
// Per slot (include/ka9q_hip.h, kq_fsk_*): q = the input quantised to int16, y = hq * q in int32, d[n] = (2 y[n] > max + min
// of y over the last W samples), a shift DPLL that takes a channel bit per symbol, descrambler, NRZI, HDLC deframer with
// the CRC-16/X.25 check.  All integer after the quantiser, so nothing depends on the order of a sum.  State on the device,
// per slot: the last HN = K - 1 + W - 1 + 63 values of q (two copies, written in turn: a call reads one and writes the other),
// the call's d packed 64 samples to a word, FskState, the open frame, the arena of good frames.
//
// k_fsk_front  kq_fskfront.hpp, shared with kq_pag: quantiser, FIR, threshold, the decisions packed 64 to a word; so is
//              the step of the bit clock
// k_fsk_track  one lane per slot: the call's words in order through DPLL, descrambler, NRZI and deframer; frames and status
//              out.  Serial by nature, as k_rds_track is; the open frame lives in global memory, written a byte at a time
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
using FskGeom = kq::fskfront::Geom;

struct FskPar {  // per slot, written by the host at kq_fsk_set
  int active;
  unsigned source;
  int scrambled;
  int min_bytes;
};

struct FskState {  // per slot, carried from call to call; all zero when a slot is set
  int s;                         // the bit clock
  unsigned sr;                   // descrambler
  int dprev, uprev;
  int ones, in_frame, nbits;
  unsigned cur;                  // the open byte
  unsigned crc_run, crc_byte;    // CRC register over the bits appended so far / at the last byte boundary
  unsigned bits, frames_good, frames_bad, aborts, dropped;
  int pad;
};

struct FskLim {  // the arena's sizes
  int max_frames, mfb;
};

struct CallArgs {
  kq::fskfront::FrontArgs<FskPar> f;   // the front end's; k_fsk_track reads its geometry, list, dw, level, n0, n1, w0
  FskLim lim;
  FskState *state;               // [S]
  unsigned char *open;           // [S][mfb]
  unsigned char *frames;         // [S][max_frames][mfb]
  kq_fsk_frame_info *info;       // [S][max_frames]
  unsigned *nframes;             // [S]
  // output
  kq_fsk_status *st;
  size_t sstride;
};

struct FrameOut {
  unsigned char *open;
  unsigned char *frames;
  kq_fsk_frame_info *info;
  unsigned n;                    // frames in the arena
};

__device__ __forceinline__ void append(FskState &s, unsigned bit, int mfb, unsigned char *open) {
  if (s.nbits < 8 * mfb) {
    s.cur |= bit << (s.nbits & 7);
    s.crc_run = (s.crc_run >> 1) ^ (((s.crc_run ^ bit) & 1u) ? 0x8408u : 0u);
    if ((s.nbits & 7) == 7) {
      open[s.nbits >> 3] = (unsigned char)s.cur;
      s.cur = 0;
      s.crc_byte = s.crc_run;
    }
  }
  if (s.nbits < 0x7FFFFFFF) s.nbits++;
}

// one data bit through the deframer (the header's "HDLC")
__device__ __forceinline__ void push_bit(FskState &s, unsigned b, FskPar const &p, FskLim const &g, FrameOut &o, int64_t n) {
  if (b) {
    if (s.ones < 7) s.ones++;
    if (s.ones == 7) {
      if (s.in_frame) s.aborts++;
      s.in_frame = 0;
    } else if (s.in_frame) {
      append(s, 1u, g.mfb, o.open);
    }
    return;
  }
  if (s.ones == 6) {
    int const nb = s.nbits - 7;
    if (s.in_frame && nb >= 8 * p.min_bytes) {
      int const len = nb >> 3;
      if ((nb & 7) == 0 && len <= g.mfb && s.crc_byte == 0xf0b8u) {
        s.frames_good++;
        if (o.n < (unsigned)g.max_frames) {
          unsigned char *dst = o.frames + (size_t)o.n * g.mfb;
          for (int i = 0; i < len; i++) dst[i] = o.open[i];
          kq_fsk_frame_info r;
          r.length = (uint32_t)len;
          r.end_bit = s.bits;
          r.end_sample = (uint64_t)n;
          o.info[o.n] = r;
          o.n++;
        } else {
          s.dropped++;
        }
      } else {
        s.frames_bad++;
      }
    }
    s.in_frame = 1;
    s.nbits = 0;
    s.cur = 0;
    s.crc_run = s.crc_byte = 0xFFFFu;
  } else if (s.ones < 5 && s.in_frame) {
    append(s, 0u, g.mfb, o.open);
  }
  s.ones = 0;
}

// one lane per slot: the call's samples in order
__global__ __launch_bounds__(64) void k_fsk_track(CallArgs c, int nlist) {
  int const li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nlist) return;
  kq::fskfront::FrontArgs<FskPar> const &a = c.f;
  int const slot = a.list[li];
  FskGeom const &g = a.g;
  FskPar const p = a.par[slot];
  FskState s = c.state[slot];
  FrameOut o;
  o.open = c.open + (size_t)slot * c.lim.mfb;
  o.frames = c.frames + (size_t)slot * c.lim.max_frames * c.lim.mfb;
  o.info = c.info + (size_t)slot * c.lim.max_frames;
  o.n = c.nframes[slot];
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
      unsigned const cb = (unsigned)d;
      unsigned u = cb;
      if (p.scrambled) {
        u = cb ^ ((s.sr >> 16) & 1u) ^ ((s.sr >> 11) & 1u);
        s.sr = ((s.sr << 1) | cb) & 0x1FFFFu;
      }
      unsigned const b = u == (unsigned)s.uprev;
      s.uprev = (int)u;
      push_bit(s, b, p, c.lim, o, n);
    }
  }
  c.state[slot] = s;
  c.nframes[slot] = o.n;
  if (c.st) {
    kq_fsk_status r;
    r.bits = s.bits;
    r.frames_good = s.frames_good;
    r.frames_bad = s.frames_bad;
    r.aborts = s.aborts;
    r.dropped = s.dropped;
    r.pll_phase = s.s;
    r.in_frame = s.in_frame;
    r.level = a.level[slot];
    c.st[(size_t)slot * c.sstride] = r;
  }
}

}  // namespace

struct kq_fsk_bank : kq::HostSide {
  static constexpr bool kDeferred = false;
  kq_fsk_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  FskGeom g{};
  int max_frames = 0, mfb = 0;
  uint64_t n_cur = 0;
  int turn = 0;                          // the copy of the carried q the next call reads
  std::vector<short> hq;
  struct Dev {  // kq::lazy_device
    kq::SlotTable<FskPar> slots;
    kq::fskfront::FrontDev front;
    FskState *state = nullptr;
    unsigned char *open = nullptr, *frames = nullptr;
    kq::EventArena<kq_fsk_frame_info> arena;  // the frames' infos and how many there are
    kq_fsk_status *st = nullptr;         // host-memory calls
  } d;
};

namespace {

int make_device(kq_fsk_bank *b) {
  kq_fsk_config const &c = b->cfg;
  FskGeom const &g = b->g;
  auto &d = b->d;
  if (b->open_stream(c.stream)) return -1;
  size_t const S = c.max_slots;
  size_t const mf = (size_t)b->max_frames, mfb = (size_t)b->mfb;
  if (d.slots.alloc(*b, S) || d.front.alloc(*b, g, b->hq) || b->alloc(&d.state, S, true) || b->alloc(&d.open, S * mfb, true) ||
      b->alloc(&d.frames, S * mf * mfb) || d.arena.alloc(*b, S, mf))
    return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

// zero history, clock, deframer and arena (the stream is idle: callers synchronised it)
int cold_start(kq_fsk_bank *b, unsigned s) {
  if (b->d.front.cold_start(*b, b->g, s)) return -1;
  KQ_TRY(hipMemsetAsync(b->d.state + s, 0, sizeof(FskState), b->stream));
  return b->d.arena.clear(*b, s, 1);
}

}  // namespace

extern "C" {

kq_fsk_bank *kq_fsk_create(const kq_fsk_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_fsk_create: null config");
    return nullptr;
  }
  kq::fskfront::FrontConfig const fc{(double)cfg->samprate, cfg->baud,        cfg->taps,      cfg->cutoff_hz,  cfg->kaiser_beta,
                                     cfg->window_bits,      cfg->input_scale, cfg->pll_shift, cfg->max_slots, cfg->max_samples};
  FskGeom g{};
  std::vector<short> hq;
  if (!kq::fskfront::front_config("kq_fsk_create", fc, &g, &hq)) return nullptr;
  if (!kq::field_in_range("kq_fsk_create", "max_frames", cfg->max_frames, 1, 4096) ||
      !kq::field_in_range("kq_fsk_create", "max_frame_bytes", cfg->max_frame_bytes, 8, 1024))
    return nullptr;
  kq_fsk_bank *b = new kq_fsk_bank;
  b->cfg = *cfg;
  b->hq = std::move(hq);
  b->g = g;
  b->max_frames = (int)cfg->max_frames;
  b->mfb = (int)cfg->max_frame_bytes;
  return b;
}

int kq_fsk_destroy(kq_fsk_bank *b) { return kq::destroy_bank(b, "kq_fsk_destroy"); }

int kq_fsk_set(kq_fsk_bank *b, unsigned slot, const kq_fsk_params *p) {
  if (!kq::set_args_ok("kq_fsk_set", slot, p, kMaxSlots)) return -1;
  if (p->min_bytes < 4) {
    kq_internal_set_error("kq_fsk_set: min_bytes %u must be >= 4", p->min_bytes);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_fsk_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (p->min_bytes > b->cfg.max_frame_bytes) {
    kq_internal_set_error("kq_fsk_set: min_bytes %u > max_frame_bytes %u", p->min_bytes, b->cfg.max_frame_bytes);
    return -1;
  }
  if (!kq::slot_in_bank("kq_fsk_set", slot, b->cfg.max_slots)) return -1;
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  KQ_TRY(hipStreamSynchronize(b->stream));
  FskPar np{};
  np.active = 1;
  np.source = p->source;
  np.scrambled = p->scrambled != 0;
  np.min_bytes = (int)p->min_bytes;
  b->d.slots.par[slot] = np;
  if (cold_start(b, slot)) return -1;
  return b->d.slots.upload(*b, slot);
}

int kq_fsk_remove(kq_fsk_bank *b, unsigned slot) { return kq::remove_slot(b, slot, "kq_fsk_remove"); }

int kq_fsk_process(kq_fsk_bank *b, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_fsk_status *status, size_t status_stride) {
  const char *fn = "kq_fsk_process";
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
  a.lim.max_frames = b->max_frames;
  a.lim.mfb = b->mfb;
  a.state = d.state;
  a.open = d.open;
  a.frames = d.frames;
  a.info = d.arena.ev;
  a.nframes = d.arena.n;
  if (kq::fskfront::launch_front(a.f, nlist, b->stream)) return -1;
  hipLaunchKernelGGL(k_fsk_track, dim3((unsigned)((nlist + 63) / 64)), dim3(64), 0, b->stream, a, (int)nlist);
  KQ_TRY(hipGetLastError());
  b->turn ^= 1;  // from here on the carried q is in the other copy, whatever fails below
  b->n_cur += ncall;
  return on_device ? 0 : kq::end_host_call(b, status, status_stride, nullptr);
}

int kq_fsk_pull_counts(kq_fsk_bank *b, uint32_t *counts) { return kq::pull_counts(b, "kq_fsk_pull_counts", counts); }

int kq_fsk_pull_frame(kq_fsk_bank *b, unsigned slot, unsigned index, unsigned char *dst, size_t cap, kq_fsk_frame_info *info) {
  const char *fn = "kq_fsk_pull_frame";
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
  kq_fsk_frame_info r;
  size_t at;
  if (kq::pull_record(b, fn, slot, index, "frames", &r, &at, scope)) return -1;
  size_t const take = std::min(cap, (size_t)r.length);
  if (take) {
    KQ_TRY(hipMemcpyAsync(dst, b->d.frames + at * b->mfb, take, hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  if (info) *info = r;
  return (int)r.length;
}

int kq_fsk_clear_frames(kq_fsk_bank *b) { return kq::clear_arena(b, "kq_fsk_clear_frames"); }

int kq_fsk_get_taps(const kq_fsk_bank *b, int16_t *dst, size_t cap) {
  if (!b) {
    kq_internal_set_error("kq_fsk_get_taps: null bank");
    return -1;
  }
  if (!dst && cap) {
    kq_internal_set_error("kq_fsk_get_taps: null dst");
    return -1;
  }
  size_t const n = std::min(cap, b->hq.size());
  if (n) std::memcpy(dst, b->hq.data(), n * sizeof(int16_t));
  return (int)b->hq.size();
}

int kq_fsk_sync(kq_fsk_bank *b) { return kq::sync_bank(b, "kq_fsk_sync"); }

int kq_fsk_reset(kq_fsk_bank *b) {
  return kq::reset_slots(b, "kq_fsk_reset", [b](unsigned s) { return cold_start(b, s); });
}

}  // extern "C"
