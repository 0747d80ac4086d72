// kq_bank.hpp -- internal to the channel bank's translation units (kq_bank*.cpp), never installed: the handle, the scopes
// its entry points open, and the functions that cross a unit boundary.
//
//   kq_bank.cpp       error text, version, create / destroy, sync / join, timing
//   kq_bank_ctl.cpp   the control plane's way to the device: write queues, response designs, compute_n0 masks, channel lists
//   kq_bank_call.cpp  one call: staging, launch decisions, the launches, the process entry points
//   kq_bank_chan.cpp  channels coming, going and changing
//   kq_bank_io.cpp    samples in (push, RTP), results out (planes, PCM, RTP, responses)
//
// Lock discipline.  One lock per handle (kq_bank::mu), taken by every entry point that reads or writes what another thread
// may change, through BankScope (or LockOnly, see there); let go of only while an entry point waits for the device, through
// Unlocked.  Everything in namespace kq::bank below wants the lock held, and the handle's device current, by its caller.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "kq_design.hpp"
#include "kq_device.hpp"
#include "kq_host.hpp"

// launch errors are sticky until read: name the launch group that failed
#define LAUNCH_CHECK(what)                                                                        \
  do {                                                                                            \
    hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess) {                                                                       \
      kq_internal_set_error("kernel launch failed in %s: %s", what, hipGetErrorString(e_));       \
      return -1;                                                                                  \
    }                                                                                             \
  } while (0)

namespace kq::bank {

// One NCO in closed form.  `frozen` mirrors osc.c:43: an oscillator whose set frequency is zero
// never advances, whatever its sweep rate.
struct Osc {
  bool init = false;
  bool frozen = true;
  double phase = 0;  // turns at sample n_ref
  double f = 0;      // cycles/sample applied between n_ref and n_ref+1
  double r = 0;      // cycles/sample^2
  double set_f = 0;  // value last passed to set() -- what osc->freq holds in the reference
  int64_t n_ref = 0;

  double phase_at(int64_t n) const {
    if (frozen) return phase;
    double const k = (double)(n - n_ref);
    return phase + f * k + r * (0.5 * k * (k - 1.0));
  }
  double step_at(int64_t n) const { return frozen ? 0.0 : f + r * (double)(n - n_ref); }
  double sweep() const { return frozen ? 0.0 : r; }
  // set_osc (osc.c:22-36): keeps the phase when already initialised
  void set(double freq, double rate, int64_t now) {
    if (init) {
      phase = phase_at(now);
      phase -= std::floor(phase);
    } else {
      phase = 0;
      init = true;
    }
    n_ref = now;
    set_f = freq;
    frozen = (freq == 0);
    f = freq;
    r = rate;
  }
  // move the reference point forward so k stays small (no change of the generated sequence)
  void rebase(int64_t now) {
    if (!init || frozen) {
      n_ref = now;
      return;
    }
    double const p = phase_at(now);
    f = step_at(now);
    phase = p - std::floor(p);
    n_ref = now;
  }
};

struct HostChan {
  kq_channel_config cfg;
  Osc lo2, dop, shift;
  // oscillators as they were before a retune that has not reached the kernels yet: the M-1 history samples of
  // the next block were mixed with these (radio.c:132-139)
  Osc lo2_old, dop_old;    // the oscillators before the last retune (the history planes) ...
  // ... and the ones before the retunes before that, while samples of theirs are still in the history: [0] the transition
  // before the last, [l + 1] the one before [l]
  Osc lo2_oldx[kq::kOldLevels], dop_oldx[kq::kOldLevels];
  bool retuned = false;
  // ... and how many samples from the start of the NEXT call's first window still carry the old oscillators (ChanDev::hist_len):
  // M - 1 when the retune happens; a call of n blocks takes n L off it; the channel stays `retuned` while any are left
  int64_t hist_old = 0;
  int64_t hist_oldx[kq::kOldLevels] = {};  // the same for lo2_oldx / dop_oldx (older: fewer samples; 0 ends the list)
  int hist_dev = -1;   // what hist_len[c] on the device was last told
  // ... and hist2_len[kOldLevels c + l]; -1 = never (the words of a slot taken over from a removed channel are whatever that
  // one left: the first retune writes every level)
  int histx_dev[kq::kOldLevels] = {-1, -1, -1, -1};
  static_assert(kq::kOldLevels == 4, "histx_dev's initialiser");
  bool active = true;  // false: a hole left by kq_bank_remove_channel, reused by the next kq_bank_add_channel
  kq_out_rtp_state out_rtp{};  // demod->output.rtp + output.silent (audio.c:32-132)
  int out_type;
  std::vector<kq::cfloat> resp, aresp;
  float noise_gain;
  int pll_slot = -1;  // carrier-tracking channels: the slot of the loop's state and ring (pll_acquire)
  int n0slot = -1;  // which of the bank's compute_n0 mask sets this channel uses (shared by all channels with its edges)
  // where the channel stands in the bank's lists (kq_bank: list_host[lk][lpos], list_active_host[apos]); lk = 3: on the
  // carrier-loop list, -1: on none
  int lk = -1, lpos = -1, apos = -1;
  bool patched = false;  // an oscillator of this channel has been set since the last call (it is on the bank's patch list)
  double r_eff = 0;      // sweep of its input oscillators as the launch decisions last saw it (cycles / sample^2)
};

struct EventPair {
  hipEvent_t a, b;
};

}  // namespace kq::bank

struct kq_bank : kq::HostSide {
  // ---- the handle: its lock, configuration and geometry, and where the sample clock stands (every unit)
  // One lock per handle, taken by every entry point: a receiver thread in its process / push / pull loop and an operator's
  // thread changing filters, modes and frequencies (display.c / radio_status.c beside the demodulator threads of the
  // reference) may share a bank.  The entry points that wait for the device to catch up (kq_bank_pull_wait, _host_io_wait,
  // _sync) let go of it while they wait.  Recursive: some entry points are built from others.
  std::recursive_mutex mu;
  kq_bank_config cfg;
  kq::Geom g;
  int fwd_mode = KQ_FWD_FULL;
  uint64_t calls = 0;
  int64_t n_abs = 0;        // absolute index of the first new (not yet processed) sample
  int64_t out_abs = 0;      // absolute index of the next output sample
  unsigned last_blocks = 0;

  // ---- the device's tables and planes that outlive a call (made by create_alloc, kq_bank.cpp; launched with by kq_bank_call.cpp)
  const float2 *tw = nullptr;  // kq::half_twiddles(g.tw_log2): shared, not the bank's to free
  float2 *chan_tw = nullptr;  // pruned path: per-channel twiddle tables
  bool chan_tw_dirty = true;
  // full-spectrum path, N = 16384: chd.row_ph (the unswept steady-state variant's row phasors, one row per channel slot) no
  // longer matches some channel's frequency step -- set wherever chan_tw_dirty is; the next call that launches that variant
  // rebuilds the plane in front of it, as does every call that stages the oscillator planes afresh
  bool row_ph_dirty = true;
  kq::ChanDev chd{};  // (what a geometry does not use stays null)
  kq::Planes pl{};
  float *energy_state = nullptr;
  float2 *win_paired = nullptr;  // row-paired copy of a call's samples for k_filter_full16k (full16k_paired_supported)
  // N = 65536 full-spectrum path (four sibling workgroups per channel-block, kq_full16k.hip): what the siblings hand to
  // each other and to k_epilogue64k; big.err is pinned host memory the kernel writes when a sibling never showed up
  bool use64k = false;
  kq::Big64 big{};
  // generic FM path: detected samples of a call [C][B][olen] and the de-emphasis filter's history [C][Mdec-1],
  // double buffered by call parity (read by every block-0 workgroup while the last block writes the next one)
  float *fmout = nullptr;
  float *fm_hist[2] = {nullptr, nullptr};
  int fm_hist_cur = 0;

  // ---- timing (kq_bank.cpp; the intervals are opened and closed by kq_bank_call.cpp and kq_bank_io.cpp through Scope)
  int timing = 0;  // 0 off, 1 filter kernel only, >= 2 every scope
  kq_host_timing host_acc = {};  // the host's own time inside the process calls (always on: three clock reads per call)
  const char *worst_holder = "";  // the entry point behind host_acc.ctl_hold_max_ms
  std::vector<kq::bank::EventPair> ev_filter, ev_demod, ev_ingest;
  size_t ev_used[3] = {0, 0, 0};
  kq_timing acc = {};

  // ---- the control plane's way to the device: write queues, design queue, compute_n0 mask slots, channel lists (kq_bank_ctl.cpp)
  // Control-plane writes (per-channel parameters, responses, carried-state resets, channel lists) do not touch the device
  // when they are made: they gather in pinned host memory, in two queues, and the next process call applies each queue with
  // ONE small launch (k_ctl_apply) at the place in the stream order where its readers expect it --
  //   FILTER side: what the filter kernels read (responses, compute_n0 masks, the ISB flag, the filter launch's lists):
  //                on the main stream in front of the call's first kernel, behind the filter passes in flight;
  //   DEMOD side:  what the demodulators read and carry (gains, flags, squelch / AGC / filter state, their lists): on
  //                whichever stream the call's demodulators run, in front of them, behind the demodulators in flight.
  // The calls in flight keep the values they were queued with, nothing waits on the host or across streams, and a
  // change costs the device a few microseconds (as separate small copies on the stream each change cost 0.5-1 ms of
  // pipeline time at 32768 channels, tools/soak_realtime.py --only filter).
  struct CtlQueue {
    static constexpr size_t kBytes = 1u << 20, kMaxRec = 4096;
    static constexpr int kDepth = 4;  // the host runs up to three calls ahead of the device (kq_bank_pull_wait's lag + 1)
    unsigned char *buf[kDepth] = {};  // pinned; [records (32 B each, kMaxRec of them) | payloads]
    hipEvent_t applied[kDepth] = {};
    bool applied_set[kDepth] = {};
    int cur = 0;
    unsigned nrec = 0;
    size_t used = 0;  // payload bytes
    // The records of one launch are applied concurrently, one workgroup each: two writes to one place must not both be in
    // it.  A later write to a destination already in the queue replaces the earlier one on the host (destination -> record).
    std::unordered_map<unsigned long long, unsigned> at;
  };
  CtlQueue ctl[2];  // 0 filter side, 1 demod side
  // Responses are designed where they are used: kq_bank_set_filter / add_channel / set_mode gather design jobs, and the
  // next call launches ONE design kernel for them on the main stream in front of its filter pass, which writes each
  // response into its channel's row (kq_design.hip design_launch).  No copy back, no wait: on a bank at real time the
  // round trip of a design on a stream of its own came to 2.0-2.4 ms of host time per operation (its packets queue
  // behind the copy kernels that share its hardware queue; tools/soak_realtime.py).  The noise gain a design yields is
  // demodulator-side state: the kernel leaves it in ng_next[epoch parity][channel] and a device-to-device record of the
  // DEMOD queue moves it over in front of the call's demodulators.  The host's copy of a response (kq_bank_get_response)
  // is fetched when asked for.
  struct DesignQueue {
    static constexpr unsigned kMax = 1024;
    static constexpr int kDepth = 4;
    unsigned char *pin[kDepth] = {};  // pinned: [kMax jobs | kMax targets]
    hipEvent_t read[kDepth] = {};     // the launch that read pin[k] is over
    bool read_set[kDepth] = {};
    int cur = 0;
    std::vector<kq::DesignJob> jobs;
    std::vector<kq::DesignTarget> targets;
    std::unordered_map<int, unsigned> at;  // channel -> job: the later design of a channel replaces the earlier one
    unsigned max_jobs = kMax;              // what the scratch holds
    float2 *scratch = nullptr;             // max_jobs * Ndec
    float *ng_next = nullptr;              // [2][max_channels]
    hipEvent_t ng_moved[2] = {};           // the DEMOD-side records that read ng_next[p] have been applied
    bool ng_moved_set[2] = {false, false};
    int ng_to_record = -1;                 // parity whose records the next DEMOD flush applies
    unsigned long long epoch = 0;
  };
  DesignQueue dq;
  std::map<float, std::vector<kq::cfloat>> aresp_cache;  // FM audio response by Kaiser beta (fm.c:54-66: geometry fixed per bank)
  // compute_n0's lane masks depend on a channel's filter edges only, and a receiver's channels mostly share a handful
  // of filters: one mask set (2 KiB; N = 65536: 8 KiB) per distinct pair of edges, counted references, so that the masks
  // of tens of thousands of channels stay in the L2 instead of streaming 70 MB per block from memory
  std::map<std::pair<float, float>, int> n0slot_of;
  std::vector<int> n0slot_refs;                       // per slot; 0 = free
  std::vector<std::pair<float, float>> n0slot_key;    // per slot
  int *list_dev[3] = {nullptr, nullptr, nullptr};  // fm, am, linear (without PLL)
  int *list_active_dev = nullptr;      // the active channels, for the filter launch, when remove_channel has left holes
  int *list_active_ds_dev = nullptr;   // the same list as the PCM stage reads it, on the demodulators' stream
  // Every active channel, in no particular order (the lists follow the channels' coming and going incrementally: a channel
  // that leaves is replaced by the list's last entry, one that comes is appended -- one or two 4-byte writes to the device's
  // copy instead of the list: at 32 768 channels a rebuilt list was 128 KiB over the link per change).  Used by the launches
  // only while there are holes (fewer entries than slots); a bank whose channels have ALL been removed never launches.
  std::vector<int> list_active_host;
  std::vector<int> list_pll_host;
  std::vector<int> list_host[3];
  bool lists_dirty = true;

  // ---- one call: the demodulators' stream, the hand-over planes, the staging slots, the oscillators' steady state and the
  // patch list, the launch decisions (kq_bank_call.cpp)
  // The demodulators are latency-bound and independent of the next batch's filter pass, so they run on a
  // second stream: filter(k+1) overlaps demod(k).  Planes the two stages hand over are double buffered.
  hipStream_t stream2 = nullptr;   // demodulators of a call that overlaps the next call's filter pass (== stream: never)
  int overlap_mode = -1;           // KQ_DEMOD_OVERLAP: 0 never, 1 always, unset (-1) per call, see run_blocks
  bool demod_overlapped[2] = {false, false};  // by call parity: ev_demod_done[parity] was recorded on stream2
  bool pulled_since_call = false;  // kq_bank_pull_planes_async since the last call: the host streams planes out
  hipEvent_t ev_demod_done[2] = {nullptr, nullptr};
  kq::Planes pl2[2] = {};
  double *osc_dev2[2] = {nullptr, nullptr};
  // per-call parameters (5 double planes of max_channels + max_blocks update flags) travel through
  // pinned staging slots so kq_bank_process never has to synchronise the stream
  static constexpr int kSlots = 4;
  unsigned char *stage_host[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  // One marker per call on the main stream, recorded behind the filter launch(es) of the call that used the slot: the
  // demodulator stream waits for it, the host waits for it before it refills the slot four calls later, and with
  // kq_bank_enable_timing it closes the filter's time interval, which stage_t0 opened (a marker costs the stream ~5 us
  // behind a long kernel, tools/marker_probe.hip; there were four per call)
  hipEvent_t stage_ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_t0[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  bool stage_timed[kSlots] = {false, false, false, false};
  // the host's side of that interval: when the opening marker was queued, how long until the closing one was, which call
  std::chrono::steady_clock::time_point stage_h0[kSlots];
  double stage_submit_ms[kSlots] = {0, 0, 0, 0};
  uint64_t stage_launch[kSlots] = {0, 0, 0, 0};
  int stage_next = 0;
  size_t stage_bytes = 0;
  // Steady state of the oscillators: nothing has been set, added or removed since the call before, so the per-call planes
  // follow from that call's on the device (k_block_energy_sum) and the host touches no per-channel state at all.
  // osc_dirty = false promises: the planes of the call before are valid for its window start (planes_n_w, planes_out_abs),
  // no channel has `retuned` set, and the cached launch decisions below still hold.
  bool osc_dirty = true;
  int64_t planes_n_w = 0, planes_out_abs = 0, rebased_at = 0;
  size_t refresh_next = 0;  // the channel whose closed forms the next steady call re-references first
  std::vector<int> ret_host;  // the channels whose windows of the call being staged hold samples of an old oscillator
  bool cache_any = false;
  // Retunes (kq_bank_set_second_lo / _doppler / _shift) leave the steady state intact: the channels touched since the last
  // call are on patch_list, and the next call advances everybody on the device as usual and then overwrites just those
  // channels' planes from a few records staged by the host (the patch role of k_block_energy_sum) -- a receiver that tracks Doppler on thousands
  // of channels retunes some of them before almost every call, and staging all channels for that cost 55 us and 0.4 ms of
  // host time per call at 32768 channels.  Beyond kMaxPatch channels per call the whole bank is staged as before.
  static constexpr int kMaxPatch = 1024;
  static constexpr size_t kPatchBytes = 72;  // one record: channel index (8 bytes), then the channel's eight plane values
  std::vector<int> patch_list;
  size_t patch_off = 0;                       // of the patch records inside a staging slot
  size_t bits_off = 0;                        // of the patched-channel bitmap (one bit per channel) behind them: the threads of
                                              // k_block_energy_sum that advance the planes skip the channels its patch role writes
  std::vector<unsigned> slot_bit_words[4];    // which words of a slot's bitmap are not zero (cleared when the slot comes round)
  int n_swept = 0, n_fast = 0;                // active channels with a sweep / with one beyond the table path's reach (N = 65536
                                              // and N = 16384: full64k_sweep_limit / full16k_sweep_limit)
  int n_active = 0;
  // N = 16384, some channels swept (satellite passes in a bank of fixed-frequency channels): the unswept ones still run the
  // steady-state variant of the kernel (16-byte loads from the row-paired copy, no per-sample oscillator path), the swept
  // ones the general variant, as two launches over two channel lists -- one swept channel used to cost the whole bank 6 %
  int *list_unswept_dev = nullptr, *list_swept_dev = nullptr;
  std::vector<int> list_unswept_host, list_swept_host;
  bool sweep_lists_dirty = true;

  // ---- the channels and the carrier loops' slots (kq_bank_chan.cpp)
  std::vector<kq::bank::HostChan> chans;
  // carrier-tracking linear channels (linear.c:129-246): own list, 65536-sample search ring per channel
  // carrier-tracking channels: a slot each (state + 65536-sample ring + search scratch), handed out from chunks of
  // kq::kPllChunk that are allocated as the count grows; a slot stays with its channel until the channel leaves the set, so
  // adding or removing one moves nothing and waits for nothing (rounds 1-5: slot = rank, 64 at most, synchronous moves)
  static constexpr int kMaxPllChunks = 1024;
  int *list_pll_dev = nullptr;         // [max_channels]
  int *pll_slot_dev = nullptr;         // [max_channels] channel -> slot
  kq::PllChunk *pll_chunks_dev = nullptr;  // [kMaxPllChunks]
  std::vector<kq::PllChunk> pll_chunks;
  std::vector<int> pll_free;           // slots not in use, lowest last

  // ---- samples in, results out: the ring and its packet bookkeeping, streaming host I/O, PCM and spectrum capture (kq_bank_io.cpp)
  float2 *ring[2] = {nullptr, nullptr};
  int cur = 0;
  size_t ring_cap = 0;   // samples, including the M-1 history
  size_t pending = 0;    // new samples in the ring beyond the history
  std::vector<unsigned char> zero_tail;  // per pending block: 1 if its last sample came from a zero fill
  size_t zero_run = 0;                   // trailing zero-fill samples of the partially filled block
  bool partial_ends_in_zero = false;
  // front-end packet bookkeeping (struct rtp_state + demod->input.samples)
  kq_rtp_counters rtp{};
  bool rtp_init = false;
  bool rtp_retry = false;          // the last datagram was sent back with -2: the same one comes again
  uint16_t rtp_retry_seq = 0;
  uint32_t rtp_retry_ts = 0;
  unsigned char *stage_dev = nullptr;  // staging for host-side raw I/Q before conversion
  size_t stage_cap = 0;
  // streaming host I/O (kq_bank_push_iq_async / kq_bank_pull_planes_async): copy streams of their own, two input staging
  // buffers, events that order them against the kernels
  hipStream_t copy_in = nullptr, copy_out = nullptr;
  unsigned char *in_stage[2] = {nullptr, nullptr};
  size_t in_stage_cap[2] = {0, 0};
  bool in_used[2] = {false, false};  // in_ready[k] has been recorded at least once
  hipEvent_t in_ready[2] = {nullptr, nullptr}, in_free[2] = {nullptr, nullptr};
  int in_next = 0;
  // kq_bank_push_rtp's payloads gather in pinned host memory and travel as ONE asynchronous copy + conversion per run of
  // packets (flushed by kq_bank_process and by whatever else touches the ring): a datagram no longer costs a host wait
  // for everything the stream has queued -- with process calls of 1.5 ms in flight that wait was the end of real time
  unsigned char *acc_pin[2] = {nullptr, nullptr};
  size_t acc_cap = 0;        // bytes, each buffer
  int acc_cur = 0, acc_fmt = -1;
  size_t acc_n = 0;          // samples gathered in acc_pin[acc_cur]
  size_t acc_ring_off = 0;   // where in the ring (samples) the run starts
  hipEvent_t acc_read[2] = {nullptr, nullptr};  // the copy engine has read the buffer
  bool acc_read_set[2] = {false, false};
  hipEvent_t out_ready = nullptr;
  // one marker per queued plane copy, a ring of them: the next call's demodulators wait for the newest on the device, and a
  // streaming host waits for the one `lag` deliveries back (kq_bank_pull_wait) while newer calls are in flight
  static constexpr int kPullRing = 8;
  hipEvent_t pull_done[kPullRing] = {};
  uint64_t pulls = 0;        // plane copies queued so far; the newest one's marker is pull_done[(pulls - 1) % kPullRing]
  bool out_pending = false;  // a plane copy is queued that the next call's demodulators must wait for
  float2 *spec_dump = nullptr;
  int spec_ch = -1;
  bool pcm_on = false;
  short *pcm = nullptr;       // [C][max_blocks][2*olen] int16, network byte order
  unsigned *pcm_mask = nullptr;  // [C][max_blocks]
};

namespace kq::bank {

// a buffer made after create, cleared before the call returns: whichever of the bank's streams reads it first finds zeros
template <typename T>
int alloc_cleared(kq_bank *b, T **p, size_t n) {
  if (b->alloc(p, n)) return -1;
  KQ_TRY(hipMemset(*p, 0, n * sizeof(T)));
  return 0;
}

inline bool valid_ch(const kq_bank *b, int ch) { return b && ch >= 0 && (size_t)ch < b->chans.size() && b->chans[ch].active; }

// the sweep beyond which a channel is `fast` (kq_bank::n_fast): out of reach of the table path of the bank's full-spectrum kernel
inline double sweep_limit(const kq_bank *b) { return b->use64k ? kq::full64k_sweep_limit() : kq::full16k_sweep_limit(); }

// How the entry points take the handle's lock.
//  * BankScope: every entry point but the ones named below.  The device switch, the lock, and the lock figures of
//    kq_host_timing.  The entry points that let go of it while they wait for the device (Unlocked): kq_bank_pull_wait,
//    kq_bank_host_io_wait, kq_bank_sync, and the three process calls for their staging slot (slot_prewait).
//  * LockOnly: kq_bank_channel_active, _num_channels, _blocks_ready, _rtp_from_planes, _get_host_timing, _worst_lock_holder.
//    Host state only, so no device switch; and no hold-time accounting -- they are what a receiver polls between calls, and
//    _get_host_timing / _worst_lock_holder read the very figures a BankScope would write on its way out.
//  * No lock at all: kq_bank_olen, _last_blocks, _stream, _audio_device_ptr, _status_device_ptr, _fwd_mode.  olen, the
//    stream, the audio and status planes and the forward mode are fixed at create, so any thread may ask at any time;
//    _last_blocks is one word the process calls write: a thread other than the receiver's reads some call's value, no more.
//    kq_bank_destroy takes none either: nobody else may be using a handle that is being destroyed.
struct LockOnly {
  std::lock_guard<std::recursive_mutex> lk;
  explicit LockOnly(const kq_bank *b) : lk(const_cast<kq_bank *>(b)->mu) {}
};
// every other entry point taking a handle: the handle's device made current, the handle's lock held.
// kq_host_timing's lock figures are kept here: a `receiver` scope (the process calls) records how long it WAITED for the
// lock, every other scope how long it HELD it (device waits taken with the lock let go -- Unlocked -- not counted): the
// worst of the second is the longest the receiver thread can have been kept out by the control plane.
struct BankScope {
  using clock = std::chrono::steady_clock;
  kq::DeviceScope dev;
  std::unique_lock<std::recursive_mutex> lk;
  kq_bank *bank = nullptr;
  bool receiver = false;
  const char *who;  // the entry point (its function name, taken where the scope is declared)
  clock::time_point t_acq;
  double unlocked_ms = 0;
  explicit BankScope(kq_bank *b, bool receiver_ = false, const char *fn = __builtin_FUNCTION())
      : dev(b ? b->cfg.device : -1), bank(b), receiver(receiver_), who(fn) {
    if (!b) return;
    auto const t0 = clock::now();
    lk = std::unique_lock<std::recursive_mutex>(b->mu);
    t_acq = clock::now();
    if (receiver) {
      double const w = std::chrono::duration<double, std::milli>(t_acq - t0).count();
      b->host_acc.lock_wait_ms += w;
      if (w > b->host_acc.lock_wait_max_ms) b->host_acc.lock_wait_max_ms = w;
    }
  }
  explicit BankScope(const kq_bank *b, const char *fn = __builtin_FUNCTION()) : BankScope(const_cast<kq_bank *>(b), false, fn) {}
  ~BankScope() {
    if (!bank || receiver || !lk.owns_lock()) return;
    double const h = std::chrono::duration<double, std::milli>(clock::now() - t_acq).count() - unlocked_ms;
    if (h > bank->host_acc.ctl_hold_max_ms) {
      bank->host_acc.ctl_hold_max_ms = h;
      bank->worst_holder = who;
    }
  }
};
// a wait for the device inside an entry point: the lock is let go for its duration (one level: an entry point called from
// another keeps the outer one's)
struct Unlocked {
  BankScope &scope;
  std::unique_lock<std::recursive_mutex> &lk;
  BankScope::clock::time_point t0;
  explicit Unlocked(BankScope &s) : scope(s), lk(s.lk), t0(BankScope::clock::now()) {
    if (lk.owns_lock()) lk.unlock();
  }
  ~Unlocked() {
    if (lk.mutex() && !lk.owns_lock()) lk.lock();
    scope.unlocked_ms += std::chrono::duration<double, std::milli>(BankScope::clock::now() - t0).count();
  }
};

enum { CTL_FILTER = 0, CTL_DEMOD = 1 };
struct CtlRecHost {  // kq_ctl.hpp CtlRec
  unsigned long long dst;
  unsigned nbytes, fill, value, payload_off;  // fill: 0 payload, 1 fill with `value`, 2 copy from device address `src`
  unsigned long long src;
};
static_assert(sizeof(CtlRecHost) == 32, "control record layout");

// kq_bank.cpp
int ensure_events(kq_bank *b, std::vector<EventPair> &v, size_t need);
int report_lost_sibling(kq_bank *b);
int sync_all(kq_bank *b);
int drain_timing(kq_bank *b);
// kq_bank_ctl.cpp
int ctl_put(kq_bank *b, int side, void *dst, const void *src, size_t bytes);
int ctl_fill(kq_bank *b, int side, void *dst, unsigned value, size_t bytes);
int ctl_flush(kq_bank *b, int side, hipStream_t st);
int ctl_flush_now(kq_bank *b);
void build_n0mask(const kq_bank *b, float low, float high, std::vector<unsigned long long> &m, std::vector<unsigned> &meta);
int acquire_n0slot(kq_bank *b, float low, float high, bool *fresh);
void release_n0slot(kq_bank *b, int slot);
int upload_n0mask(kq_bank *b, int c);
// The constants each demodulator thread derives in its prologue (fm.c:86; am.c:21-30; linear.c:29-39)
struct Derived {
  int mode, flags, hangmax;
  float fm_gain, recovery, init_gain;
};
int channel_flags(const kq_channel_config &k);  // Derived::flags alone
Derived derive(const kq::Geom &g, const kq_channel_config &k);
int upload_channel(kq_bank *b, int c, bool fresh = true);
void design_edges(const kq::Geom &g, const kq_channel_config &k, bool runtime, float *lo_n, float *hi_n);
int queue_design(kq_bank *b, int c, bool runtime = false);
int fetch_response(kq_bank *b, int c);
int upload_lists(kq_bank *b);
int lists_add(kq_bank *b, int c);
int lists_retype(kq_bank *b, int c);
int lists_remove(kq_bank *b, int c, bool from_active = true);
// kq_bank_call.cpp
void harvest_slot(kq_bank *b, int slot);
void note_retune(kq_bank *b, int ch);
void note_patch(kq_bank *b, int ch);
// kq_bank_io.cpp
int acc_flush(kq_bank *b);

struct Scope {
  kq_bank *b;
  int kind;
  EventPair *p = nullptr;
  hipStream_t st;
  Scope(kq_bank *bank, int k, hipStream_t stream) : b(bank), kind(k), st(stream) {
    if (!b->timing || (kind != 0 && b->timing < 2)) return;
    std::vector<EventPair> &v = kind == 0 ? b->ev_filter : kind == 1 ? b->ev_demod : b->ev_ingest;
    if (b->ev_used[kind] >= 512) drain_timing(b);
    if (ensure_events(b, v, b->ev_used[kind] + 1)) return;
    p = &v[b->ev_used[kind]++];
    (void)hipEventRecord(p->a, st);
  }
  ~Scope() {
    if (p) (void)hipEventRecord(p->b, st);
  }
};

}  // namespace kq::bank
