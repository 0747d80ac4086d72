// kq_mon.hip -- monitor mixer bank: thousands of PCM rows, each with a gain, a stereo position and a mute switch, summed
// into stereo buses on gfx950 (monitor.c:433-450, 475-496).
//
// The definition is in include/ka9q_hip.h (kq_mon_*): a bus is the sum of its unmuted sessions in ascending slot order,
// in chunks of 64 folded by fmaf from 0.0f, the chunk partials added in chunk order.  The host keeps every session and,
// when membership or a setting changed, rebuilds three tables and uploads them at the next call: the members ordered by
// (bus, slot), the chunks (first member, count) and the buses (first chunk, count, K).  A session's history lives in a
// ring of H frames at n mod H, valid as far back as the frame the session was set at (MonRec::n_set), so a set or a
// reset costs the device nothing.
//
// k_mon_mix     one workgroup per (chunk, piece of a time tile), one thread per frame: both sides of the chunk's partial.
//               The member records are read with a uniform index (scalar loads); the input comes from the plane, or from
//               the history ring where n - d falls before the call.  Also the chunk's mask of members with a non-zero
//               input sample in this call (a wave reduction, one integer atomic OR per wave)
// k_mon_reduce  per (bus, frame): the bus's partials in chunk order, then out, pcm, peak and clip count (wave reductions,
//               integer atomics: the peak as the bits of a non-negative float)
// k_mon_status  one thread per bus: K and the population count of its chunks' masks
// k_mon_hist    after the mix, one wave per session (muted ones too): the call's last min(T, H) frames into the ring
// A call runs in time tiles of kTile frames, so the partials are [chunks][kTile] whatever max_samples is.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "ka9q_hip.h"
#include "kq_device.hpp"
#include "kq_host.hpp"
#include "kq_ldsfft.hpp"

namespace {

constexpr unsigned kMaxSessions = 65536, kMaxBuses = 256;
constexpr unsigned kChunk = 64;    // members per partial
constexpr unsigned kTile = 1024;   // frames per time tile
constexpr float kScale = 1.f / SHRT_MAX;  // monitor.c:88

struct MonRec {  // a session as the kernels see it
  unsigned source, slot;
  float gl, gr;
  unsigned delay;              // dl | dr << 16 (one of them is 0)
  unsigned stereo;
  unsigned long long n_set;    // the frame the session was set at: zero input before it
};
struct MonChunk {
  unsigned first, count;       // members first .. first + count - 1
};
struct MonBus {
  unsigned chunk0, nchunks, K, pad;
};

struct MonCall {
  const void *audio;
  int format;
  size_t src_stride, row_stride;
  unsigned block_len, T;
  const int *rowmap;           // per slot: the row of `audio` (host input, staged) or null (MonRec::source)
  float2 *hist;                // [S][H] frame n at n mod H
  unsigned H, h0;              // h0 = n0 mod H
  unsigned long long n0;       // the call's first frame
  const MonRec *mem;
  const MonChunk *chunk;
  const MonBus *bus;
  float2 *part;                // [chunks][kTile]
  unsigned long long *act;     // [chunks] bit m: member m of the chunk had a non-zero input sample
  float *out;
  size_t out_stride;
  int16_t *pcm;
  size_t pcm_stride;
  kq_mon_status *st;
};

__device__ __forceinline__ float mon_sample(const void *audio, int format, size_t idx) {
  if (format == KQ_MON_S16BE) {
    unsigned const w = reinterpret_cast<const unsigned short *>(audio)[idx];
    short const s = (short)(((w << 8) | (w >> 8)) & 0xffffu);  // ntohs
    return __fmul_rn(kScale, (float)s);                        // monitor.c:492
  }
  return reinterpret_cast<const float *>(audio)[idx];
}

// side c of x[i - d]: from the call, or from the ring as far back as the session goes.  No branch: one address is
// chosen and loaded (for int16 input one of each kind), so the loads of several members are in flight together
template <int FORMAT>
__device__ __forceinline__ float mon_fetch(const MonCall &a, const MonRec &r, size_t base, unsigned ch, unsigned i, unsigned d,
                                           unsigned c) {
  bool const now = i >= d;
  unsigned const ii = now ? i - d : 0u, k = ii / a.block_len, j = ii - k * a.block_len;
  size_t const e = base + (size_t)k * a.row_stride + (size_t)j * ch + c;
  unsigned const back = now ? 1u : d - i;  // 1 .. H
  bool const zero = !now && back > a.n0 - r.n_set;
  unsigned pos = a.h0 + a.H - back;
  if (pos >= a.H) pos -= a.H;
  const float *h = reinterpret_cast<const float *>(a.hist + (size_t)r.slot * a.H + pos) + c;
  float v;
  if constexpr (FORMAT == KQ_MON_F32) {
    v = *(now ? reinterpret_cast<const float *>(a.audio) + e : h);
  } else {
    float const p = mon_sample(a.audio, FORMAT, e), q = *h;
    v = now ? p : q;
  }
  return zero ? 0.f : v;
}

// grid (chunks, pieces of the tile); frames t0 .. t0 + tn - 1 of the call
template <int FORMAT>
__global__ __launch_bounds__(256) void k_mon_mix(MonCall a, unsigned t0, unsigned tn) {
  MonChunk const ck = a.chunk[blockIdx.x];
  unsigned const it = blockIdx.y * blockDim.x + threadIdx.x;
  bool const live = it < tn;
  unsigned const i = t0 + (live ? it : 0u);  // a lane beyond the tile repeats its first frame and stores nothing
  float accl = 0.f, accr = 0.f;
  unsigned long long act = 0;
#pragma unroll 4
  for (unsigned m = 0; m < ck.count; m++) {
    MonRec const r = a.mem[ck.first + m];
    size_t const row = a.rowmap ? (size_t)a.rowmap[r.slot] : (size_t)r.source;
    size_t const base = row * a.src_stride;
    unsigned const ch = r.stereo ? 2u : 1u;
    // the frame itself, for the test of silence; the delayed side apart (the other load repeats and hits the cache)
    float const ul = mon_fetch<FORMAT>(a, r, base, ch, i, 0, 0), ur = mon_fetch<FORMAT>(a, r, base, ch, i, 0, ch - 1);
    float const xl = mon_fetch<FORMAT>(a, r, base, ch, i, r.delay & 0xffffu, 0);
    float const xr = mon_fetch<FORMAT>(a, r, base, ch, i, r.delay >> 16, ch - 1);
    act |= (unsigned long long)(ul != 0.f || ur != 0.f) << m;  // (no ballot here: a convergent call would keep the loop rolled)
    accl = __fmaf_rn(r.gl, xl, accl);
    accr = __fmaf_rn(r.gr, xr, accr);
  }
  if (live) a.part[(size_t)blockIdx.x * kTile + it] = make_float2(accl, accr);
  auto either = [](int x, int y) { return x | y; };
  if (!live) act = 0;
  unsigned const lo = (unsigned)kq::wave_reduce((int)(unsigned)act, either), hi = (unsigned)kq::wave_reduce((int)(act >> 32), either);
  act = (unsigned long long)hi << 32 | lo;
  if ((threadIdx.x & 63) == 0 && act) atomicOr(&a.act[blockIdx.x], act);
}

// grid (pieces of the tile, buses)
__global__ __launch_bounds__(256) void k_mon_reduce(MonCall a, unsigned t0, unsigned tn) {
  unsigned const b = blockIdx.y, it = blockIdx.x * blockDim.x + threadIdx.x;
  bool const live = it < tn;
  unsigned const q = live ? it : 0u;
  MonBus const bs = a.bus[b];
  float l = 0.f, r = 0.f;
  for (unsigned c = 0; c < bs.nchunks; c++) {
    float2 const p = a.part[(size_t)(bs.chunk0 + c) * kTile + q];
    l = __fadd_rn(l, p.x);
    r = __fadd_rn(r, p.y);
  }
  unsigned const wl = kq::pcm_word_be(l), wr = kq::pcm_word_be(r);
  size_t const f = (size_t)t0 + q;
  if (live && a.out) {
    float *o = a.out + (size_t)b * a.out_stride + 2 * f;
    o[0] = l;
    o[1] = r;
  }
  if (live && a.pcm) {
    int16_t *o = a.pcm + (size_t)b * a.pcm_stride + 2 * f;
    o[0] = (int16_t)wl;
    o[1] = (int16_t)wr;
  }
  if (!a.st) return;
  // SHRT_MAX is 0x7fff, SHRT_MIN 0x8000: bytes swapped, 0xff7f and 0x0080
  auto hit = [](unsigned w) { return (int)(w == 0xff7fu || w == 0x0080u); };
  auto imax = [](int x, int y) { return x > y ? x : y; };
  int const nclip = kq::wave_sum_i(live ? hit(wl) + hit(wr) : 0);
  int const pl = kq::wave_reduce(live ? __float_as_int(fabsf(l)) : 0, imax);  // |x| as bits: ordered as integers
  int const pr = kq::wave_reduce(live ? __float_as_int(fabsf(r)) : 0, imax);
  if ((threadIdx.x & 63) == 0) {
    kq_mon_status *s = a.st + b;
    if (nclip) atomicAdd(&s->clipped, nclip);
    if (pl) atomicMax(reinterpret_cast<int *>(&s->peak_left), pl);
    if (pr) atomicMax(reinterpret_cast<int *>(&s->peak_right), pr);
  }
}

__global__ __launch_bounds__(256) void k_mon_status(MonCall a, unsigned nbuses) {
  unsigned const b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbuses) return;
  MonBus const bs = a.bus[b];
  int n = 0;
  for (unsigned c = 0; c < bs.nchunks; c++) n += __popcll(a.act[bs.chunk0 + c]);
  a.st[b].sessions = (int)bs.K;
  a.st[b].active = n;
}

// one wave per session: frames T - cnt .. T - 1 of the call into the ring from position hs, cnt = min(T, H)
__global__ __launch_bounds__(64) void k_mon_hist(MonCall a, const MonRec *__restrict__ all, unsigned cnt, unsigned hs) {
  MonRec const r = all[blockIdx.x];
  size_t const row = a.rowmap ? (size_t)a.rowmap[r.slot] : (size_t)r.source;
  size_t const base = row * a.src_stride;
  unsigned const ch = r.stereo ? 2u : 1u;
  for (unsigned q = threadIdx.x; q < cnt; q += 64) {
    unsigned const i = a.T - cnt + q, k = i / a.block_len, j = i - k * a.block_len;
    size_t const e = base + (size_t)k * a.row_stride + (size_t)j * ch;
    float const xl = mon_sample(a.audio, a.format, e);
    float const xr = r.stereo ? mon_sample(a.audio, a.format, e + 1) : xl;
    unsigned pos = hs + q;
    if (pos >= a.H) pos -= a.H;
    a.hist[(size_t)r.slot * a.H + pos] = make_float2(xl, xr);
  }
}

struct Session {
  bool used = false;
  kq_mon_params p{};
  uint64_t n_set = 0;
};

}  // namespace

struct kq_mon_bank : kq::HostSide {
  kq_mon_config cfg;
  std::mutex mu;
  bool dev_ready = false;
  unsigned H = 0, max_chunks = 0;
  uint64_t n_cur = 0;
  std::vector<Session> sess;
  unsigned nstereo = 0;          // stereo sessions set
  bool dirty = true;             // the tables below are behind `sess`
  std::vector<MonRec> mem, all;  // members by (bus, slot); every session by slot
  std::vector<MonChunk> chunk;
  std::vector<MonBus> bus;
  struct Dev {  // kq::lazy_device
    MonRec *mem = nullptr, *all = nullptr;
    MonChunk *chunk = nullptr;
    MonBus *bus = nullptr;
    float2 *part = nullptr, *hist = nullptr;
    unsigned long long *act = nullptr;
    kq_mon_status *st = nullptr;
    // host-memory calls
    int *rowmap = nullptr;
    char *stage = nullptr;
    size_t stage_cap = 0;  // bytes
    float *out = nullptr;
    size_t out_cap = 0;
    int16_t *pcm = nullptr;
    size_t pcm_cap = 0;
  } d;
  std::vector<int> rowmap;  // host-memory calls
};

namespace {

int make_device(kq_mon_bank *b) {
  if (b->open_stream(b->cfg.stream)) return -1;
  size_t const S = b->cfg.max_sessions, B = b->cfg.max_buses, C = b->max_chunks;
  if (b->alloc(&b->d.mem, S) || b->alloc(&b->d.all, S) || b->alloc(&b->d.chunk, C) || b->alloc(&b->d.bus, B) ||
      b->alloc(&b->d.part, C * kTile) || b->alloc(&b->d.act, C) || b->alloc(&b->d.hist, S * b->H) || b->alloc(&b->d.st, B))
    return -1;
  return 0;
}

void delays(const kq_mon_config &c, float pan, unsigned *dl, unsigned *dr) {
  *dl = pan > 0 ? (unsigned)std::round((double)pan * .001 * c.samprate) : 0u;   // monitor.c:444-447
  *dr = pan < 0 ? (unsigned)std::round(-(double)pan * .001 * c.samprate) : 0u;
}

// the tables from `sess`, and their upload on the stream; waits, so the host copies may change again
int rebuild(kq_mon_bank *b) {
  unsigned const S = b->cfg.max_sessions, B = b->cfg.max_buses;
  std::vector<unsigned> count(B + 1, 0);
  b->all.clear();
  for (unsigned s = 0; s < S; s++) {
    Session const &x = b->sess[s];
    if (!x.used) continue;
    MonRec r{};
    r.source = x.p.source;
    r.slot = s;
    r.gl = x.p.gain * (1 - x.p.pan) / 2;  // monitor.c:440-441, in float
    r.gr = x.p.gain * (1 + x.p.pan) / 2;
    unsigned dl, dr;
    delays(b->cfg, x.p.pan, &dl, &dr);
    r.delay = dl | dr << 16;
    r.stereo = x.p.channels == 2;
    r.n_set = x.n_set;
    b->all.push_back(r);
    if (!x.p.muted) count[x.p.bus + 1]++;
  }
  for (unsigned k = 0; k < B; k++) count[k + 1] += count[k];
  b->mem.assign(count[B], MonRec{});
  {
    std::vector<unsigned> at(count.begin(), count.end() - 1);
    for (MonRec const &r : b->all) {
      kq_mon_params const &p = b->sess[r.slot].p;
      if (!p.muted) b->mem[at[p.bus]++] = r;
    }
  }
  b->chunk.clear();
  b->bus.assign(B, MonBus{});
  for (unsigned k = 0; k < B; k++) {
    unsigned const K = count[k + 1] - count[k];
    b->bus[k].chunk0 = (unsigned)b->chunk.size();
    b->bus[k].nchunks = (K + kChunk - 1) / kChunk;
    b->bus[k].K = K;
    for (unsigned m = 0; m < K; m += kChunk) b->chunk.push_back(MonChunk{count[k] + m, std::min(kChunk, K - m)});
  }
  auto up = [b](auto *dst, auto const &v) {
    if (v.empty()) return hipSuccess;
    return hipMemcpyAsync(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, b->stream);
  };
  KQ_TRY(up(b->d.mem, b->mem));
  KQ_TRY(up(b->d.all, b->all));
  KQ_TRY(up(b->d.chunk, b->chunk));
  KQ_TRY(up(b->d.bus, b->bus));
  KQ_TRY(hipStreamSynchronize(b->stream));
  b->dirty = false;
  return 0;
}

const char *check_gain_pan(float gain, float pan) {
  if (!std::isfinite(gain) || gain < 0) return "gain must be finite and >= 0";
  if (!std::isfinite(pan) || std::fabs(pan) > 1) return "pan must be -1 .. +1";
  return nullptr;
}

}  // namespace

extern "C" {

kq_mon_bank *kq_mon_create(const kq_mon_config *cfg) {
  if (!cfg) {
    kq_internal_set_error("kq_mon_create: null config");
    return nullptr;
  }
  if (cfg->samprate < 8000 || cfg->samprate > 384000) {
    kq_internal_set_error("kq_mon_create: samprate %d must be 8000..384000", cfg->samprate);
    return nullptr;
  }
  if (cfg->max_sessions == 0 || cfg->max_sessions > kMaxSessions) {
    kq_internal_set_error("kq_mon_create: max_sessions %u must be 1..%u", cfg->max_sessions, kMaxSessions);
    return nullptr;
  }
  if (cfg->max_buses == 0 || cfg->max_buses > kMaxBuses) {
    kq_internal_set_error("kq_mon_create: max_buses %u must be 1..%u", cfg->max_buses, kMaxBuses);
    return nullptr;
  }
  if (cfg->max_samples == 0 || cfg->max_samples > ((size_t)1 << 28)) {
    kq_internal_set_error("kq_mon_create: max_samples %zu must be 1..2^28", cfg->max_samples);
    return nullptr;
  }
  kq_mon_bank *b = new kq_mon_bank;
  b->cfg = *cfg;
  b->H = (unsigned)std::round(.001 * cfg->samprate);
  b->max_chunks = cfg->max_sessions / kChunk + cfg->max_buses;  // >= sum over the buses of ceil(K / 64)
  b->sess.assign(cfg->max_sessions, Session{});
  return b;
}

int kq_mon_destroy(kq_mon_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mon_destroy: null bank");
    return -1;
  }
  if (b->dev_ready) {
    kq::DeviceScope dev_scope_(b->cfg.device);
    b->close();
  }
  delete b;
  return 0;
}

int kq_mon_set(kq_mon_bank *b, unsigned slot, const kq_mon_params *p) {
  if (slot >= kMaxSessions) {
    kq_internal_set_error("kq_mon_set: slot %u is beyond any bank (%u sessions at most)", slot, kMaxSessions);
    return -1;
  }
  if (!p) {
    kq_internal_set_error("kq_mon_set: null params");
    return -1;
  }
  if (p->channels != 1 && p->channels != 2) {
    kq_internal_set_error("kq_mon_set: channels %d must be 1 or 2", p->channels);
    return -1;
  }
  if (const char *why = check_gain_pan(p->gain, p->pan)) {
    kq_internal_set_error("kq_mon_set: %s", why);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_mon_set: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_sessions) {
    kq_internal_set_error("kq_mon_set: slot %u >= max_sessions %u", slot, b->cfg.max_sessions);
    return -1;
  }
  if (p->bus >= b->cfg.max_buses) {
    kq_internal_set_error("kq_mon_set: bus %u >= max_buses %u", p->bus, b->cfg.max_buses);
    return -1;
  }
  Session &x = b->sess[slot];
  if (x.used && x.p.channels == 2) b->nstereo--;
  x.used = true;
  x.p = *p;
  x.p.muted = p->muted ? 1 : 0;
  x.n_set = b->n_cur;
  if (p->channels == 2) b->nstereo++;
  b->dirty = true;
  return 0;
}

int kq_mon_adjust(kq_mon_bank *b, unsigned slot, float gain, float pan, int muted) {
  if (const char *why = check_gain_pan(gain, pan)) {
    kq_internal_set_error("kq_mon_adjust: %s", why);
    return -1;
  }
  if (!b) {
    kq_internal_set_error("kq_mon_adjust: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_sessions || !b->sess[slot].used) {
    kq_internal_set_error("kq_mon_adjust: slot %u holds no session", slot);
    return -1;
  }
  kq_mon_params &p = b->sess[slot].p;
  p.gain = gain;
  p.pan = pan;
  p.muted = muted ? 1 : 0;
  b->dirty = true;
  return 0;
}

int kq_mon_remove(kq_mon_bank *b, unsigned slot) {
  if (!b) {
    kq_internal_set_error("kq_mon_remove: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (slot >= b->cfg.max_sessions || !b->sess[slot].used) {
    kq_internal_set_error("kq_mon_remove: slot %u holds no session", slot);
    return -1;
  }
  if (b->sess[slot].p.channels == 2) b->nstereo--;
  b->sess[slot] = Session{};
  b->dirty = true;
  return 0;
}

int kq_mon_process(kq_mon_bank *b, const void *audio, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, float *out, size_t out_stride, int16_t *pcm, size_t pcm_stride,
                   kq_mon_status *status) {
  if (!b) {
    kq_internal_set_error("kq_mon_process: null bank");
    return -1;
  }
  if (format != KQ_MON_F32 && format != KQ_MON_S16BE) {
    kq_internal_set_error("kq_mon_process: unknown format %d", format);
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  size_t const T = (size_t)block_len * nblocks;
  if (T > b->cfg.max_samples) {
    kq_internal_set_error("kq_mon_process: nblocks %u x block_len %u = %zu > max_samples %zu", nblocks, block_len, T,
                          b->cfg.max_samples);
    return -1;
  }
  size_t const width = (size_t)block_len * (b->nstereo ? 2 : 1);  // elements of the widest session's block
  if (nblocks > 1 && row_stride < width) {
    kq_internal_set_error("kq_mon_process: row_stride %zu < %zu, a block of block_len %u frames%s", row_stride, width, block_len,
                          b->nstereo ? " of a stereo session" : "");
    return -1;
  }
  if (out && out_stride < 2 * T) {
    kq_internal_set_error("kq_mon_process: out_stride %zu < 2 T = %zu", out_stride, 2 * T);
    return -1;
  }
  if (pcm && pcm_stride < 2 * T) {
    kq_internal_set_error("kq_mon_process: pcm_stride %zu < 2 T = %zu", pcm_stride, 2 * T);
    return -1;
  }
  if (T == 0) return 0;
  if (!audio) {
    kq_internal_set_error("kq_mon_process: null audio");
    return -1;
  }
  kq::DeviceScope dev_scope_(b->cfg.device);
  if (kq::lazy_device(b, make_device)) return -1;
  if (b->dirty && rebuild(b)) return -1;
  unsigned const B = b->cfg.max_buses, H = b->H;
  size_t const nall = b->all.size(), nchunk = b->chunk.size(), es = format == KQ_MON_S16BE ? 2 : 4;
  MonCall a{};
  a.format = format;
  a.block_len = block_len;
  a.T = (unsigned)T;
  a.hist = b->d.hist;
  a.H = H;
  a.h0 = (unsigned)(b->n_cur % H);
  a.n0 = b->n_cur;
  a.mem = b->d.mem;
  a.chunk = b->d.chunk;
  a.bus = b->d.bus;
  a.part = b->d.part;
  a.act = b->d.act;
  if (on_device) {
    a.audio = audio;
    a.src_stride = src_stride;
    a.row_stride = nblocks > 1 ? row_stride : 0;
    a.rowmap = nullptr;
    a.out = out;
    a.out_stride = out_stride;
    a.pcm = pcm;
    a.pcm_stride = pcm_stride;
    a.st = status;
  } else {
    // the distinct source rows of the sessions, staged as [row][block][2 block_len]; of each block, what its widest reader takes
    std::map<unsigned, std::pair<int, unsigned>> rows;  // source -> (staged row, channels)
    b->rowmap.assign(b->cfg.max_sessions, 0);
    for (MonRec const &r : b->all) {
      auto it = rows.find(r.source);
      if (it == rows.end()) it = rows.emplace(r.source, std::make_pair((int)rows.size(), 1u)).first;
      if (r.stereo) it->second.second = 2;
      b->rowmap[r.slot] = it->second.first;
    }
    // (grow waits for the stream, which is idle here: the last host-memory call ended in a synchronise)
    if (b->grow(&b->d.stage, &b->d.stage_cap, std::max<size_t>(rows.size(), 1) * 2 * b->cfg.max_samples * 4)) return -1;
    if (!b->d.rowmap && b->alloc(&b->d.rowmap, b->cfg.max_sessions)) return -1;
    for (auto const &kv : rows) {
      size_t const w = (size_t)kv.second.second * block_len * es;
      KQ_TRY(hipMemcpy2DAsync(b->d.stage + (size_t)kv.second.first * 2 * T * es, (size_t)2 * block_len * es,
                               (const char *)audio + (size_t)kv.first * src_stride * es, (nblocks > 1 ? row_stride * es : w), w,
                               nblocks, hipMemcpyHostToDevice, b->stream));
    }
    KQ_TRY(hipMemcpyAsync(b->d.rowmap, b->rowmap.data(), b->rowmap.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    a.audio = b->d.stage;
    a.src_stride = 2 * T;
    a.row_stride = (size_t)2 * block_len;
    a.rowmap = b->d.rowmap;
    if (out && b->grow(&b->d.out, &b->d.out_cap, (size_t)B * 2 * T)) return -1;
    if (pcm && b->grow(&b->d.pcm, &b->d.pcm_cap, (size_t)B * 2 * T)) return -1;
    a.out = out ? b->d.out : nullptr;
    a.pcm = pcm ? b->d.pcm : nullptr;
    a.out_stride = a.pcm_stride = 2 * T;
    a.st = status ? b->d.st : nullptr;
  }
  if (a.st) KQ_TRY(hipMemsetAsync(a.st, 0, B * sizeof(kq_mon_status), b->stream));
  if (nchunk) KQ_TRY(hipMemsetAsync(b->d.act, 0, nchunk * sizeof(unsigned long long), b->stream));
  for (size_t t0 = 0; t0 < T; t0 += kTile) {
    unsigned const tn = (unsigned)std::min<size_t>(kTile, T - t0), nthr = tn <= 64 ? 64 : 256, pieces = (tn + nthr - 1) / nthr;
    if (nchunk) {
      auto mix = format == KQ_MON_S16BE ? k_mon_mix<KQ_MON_S16BE> : k_mon_mix<KQ_MON_F32>;
      hipLaunchKernelGGL(mix, dim3((unsigned)nchunk, pieces), dim3(nthr), 0, b->stream, a, (unsigned)t0, tn);
      KQ_TRY(hipGetLastError());
    }
    if (a.out || a.pcm || a.st) {
      hipLaunchKernelGGL(k_mon_reduce, dim3(pieces, B), dim3(nthr), 0, b->stream, a, (unsigned)t0, tn);
      KQ_TRY(hipGetLastError());
    }
  }
  if (a.st) {
    hipLaunchKernelGGL(k_mon_status, dim3((B + 255) / 256), dim3(256), 0, b->stream, a, B);
    KQ_TRY(hipGetLastError());
  }
  if (nall) {
    unsigned const cnt = (unsigned)std::min<size_t>(T, H), hs = (unsigned)((b->n_cur + (T - cnt)) % H);
    hipLaunchKernelGGL(k_mon_hist, dim3((unsigned)nall), dim3(64), 0, b->stream, a, b->d.all, cnt, hs);
    KQ_TRY(hipGetLastError());
  }
  if (!on_device) {
    if (out)
      KQ_TRY(hipMemcpy2DAsync(out, out_stride * sizeof(float), b->d.out, 2 * T * sizeof(float), 2 * T * sizeof(float), B,
                               hipMemcpyDeviceToHost, b->stream));
    if (pcm)
      KQ_TRY(hipMemcpy2DAsync(pcm, pcm_stride * sizeof(int16_t), b->d.pcm, 2 * T * sizeof(int16_t), 2 * T * sizeof(int16_t), B,
                               hipMemcpyDeviceToHost, b->stream));
    if (status) KQ_TRY(hipMemcpyAsync(status, b->d.st, B * sizeof(kq_mon_status), hipMemcpyDeviceToHost, b->stream));
    KQ_TRY(hipStreamSynchronize(b->stream));
  }
  b->n_cur += T;  // only once everything is queued: a call that fails leaves the frame index where it was
  return (int)T;
}

int kq_mon_sync(kq_mon_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mon_sync: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->dev_ready) return 0;
  kq::DeviceScope dev_scope_(b->cfg.device);
  KQ_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int kq_mon_reset(kq_mon_bank *b) {
  if (!b) {
    kq_internal_set_error("kq_mon_reset: null bank");
    return -1;
  }
  std::lock_guard<std::mutex> lk(b->mu);
  b->n_cur = 0;
  for (Session &x : b->sess) x.n_set = 0;  // nothing of the ring is valid: no device work
  b->dirty = true;
  return 0;
}

}  // extern "C"
