/* ka9q_hip.h -- C ABI of libka9q_hip.so: the MI355X (gfx950) implementation of ka9q-radio's
 * per-channel DSP hot path (NCO mix -> overlap-save filter/decimator -> FM / AM / linear demod).
 *
 * Plain C: pointers, sizes, ints and doubles only.  No HIP or torch types appear here; device
 * pointers and streams cross the boundary as void*.
 *
 * Two surfaces:
 *   1. kq_bank_*   -- the batched "channel bank": many receiver channels share one front-end I/Q
 *                     stream.  This is what a multi-channel `radio` binds.  Each
 *                     entry point cites the reference interface it replaces (paths relative to
 *                     the reference tree).
 *   2. compat      -- the reference's own filter.h / osc.h symbol names, one channel per object,
 *                     in ka9q_hip_compat.h.
 *
 * Error convention follows the reference (filter.c:148-149, 504-505): int functions return 0 on
 * success and -1 on a NULL / NaN / out-of-range argument; constructors return NULL on failure.
 * kq_last_error() adds a human-readable reason (the reference has none).
 */
#ifndef KA9Q_HIP_H
#define KA9Q_HIP_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum demod_type of radio.h:20-24 */
enum kq_demod_type { KQ_LINEAR_DEMOD = 0, KQ_AM_DEMOD = 1, KQ_FM_DEMOD = 2 };

/* I/Q sample formats accepted by kq_bank_push_iq:
 *   KQ_IQ_CF32 : complex float (re,im)           -- the synthetic configs of BASELINE.json
 *   KQ_IQ_S16  : int16 little-endian I,Q  (RTP payload type IQ_PT  = 97, multicast.h:19; radio.c:113-114)
 *   KQ_IQ_S8   : int8 I,Q                 (RTP payload type IQ_PT8 = 98, multicast.h:20; radio.c:117-118) */
enum kq_iq_format { KQ_IQ_CF32 = 0, KQ_IQ_S16 = 1, KQ_IQ_S8 = 2 };

/* Forward-transform strategy of the pre-detection filter */
enum kq_fwd_mode {
  KQ_FWD_AUTO = 0,    /* pruned when the geometry allows and n0 is off, else full */
  KQ_FWD_FULL = 1,    /* N-point FFT per channel in LDS, all N bins (needed by compute_n0) */
  KQ_FWD_PRUNED = 2   /* only the N/D bins execute_filter_output reads (filter.c:206-227) */
};

typedef struct kq_bank kq_bank;   /* opaque */
/* Threads: a handle carries one lock, taken by every kq_bank_* entry point, so a receiver thread (process / push / pull) and
 * an operator's thread (set_filter, set_mode, the frequency setters, add / remove -- display.c and radio_status.c beside the
 * demodulator threads of the reference) may share a bank.  The entry points whose job is to wait for the device --
 * kq_bank_pull_wait, kq_bank_host_io_wait, kq_bank_sync -- let go of the lock while they wait.  kq_last_error is per thread.
 * kq_bank_destroy wants the handle to itself.  Buffers handed to the asynchronous pulls are the caller's to keep apart. */

/* Bank geometry: replaces the arguments of create_filter_input(L, M, COMPLEX) (filter.c:54,
 * called from main.c:232) plus demod->filter.decimate and demod->input.samprate
 * (radio_status.c:264-267), which the reference keeps per process.
 * Limits (deviations from the reference, which hands any L / M to FFTW -- main.c:160-170, filter.c:78,132):
 *   - N = L + M - 1 and N / decimate: powers of two (the reference's default, N = 8192, is one), or -- since round 6, on
 *     the generic kernels -- any even 2^a 3^b 5^c 7^d up to 16384 (up to 65536 without compute_n0, where N splits into a few
 *     transforms of at most 16384 points: 24000, 38400, 48000 ...): the sizes of a front end whose rate is not 48 kHz x 2^k
 *     (decimate = samprate / 48000, radio_status.c:266: 5 at 240 kHz with L = 4800, M = 4801).  A prime factor beyond 7 is
 *     refused.  decimate must divide N, L and M - 1 (the reference only warns when it does not, filter.c:106-107); decimate 1
 *     (a 48 kHz front end) needs N <= 8192.  The fast
 *     kernels (N = 16384 / 65536 full-spectrum, the pruned ones, N/D = 64 and 256 demodulators) are power-of-two only;
 *   - the full-spectrum forward path (compute_n0 = 1) serves N <= 16384 and N = 65536; N = 32768 only without compute_n0.
 *     At N = 65536 the four workgroups of a channel-block wait for each other (bounded: a lost one gives NaN and an error
 *     from kq_bank_sync, never a hung device): run such banks from ONE process per GPU -- two processes' launches in flight on
 *     one device can starve each other's workgroups until the waits run out;
 *   - carrier-tracking channels (kq_channel_config.pll, linear.c:129-246): as many as the bank has channels, up to 65536;
 *     each keeps a 65536-sample search ring (544 KiB with its state), allocated 64 channels at a time as the count grows;
 *   - the PL-tone measurement (fm.c:201-205 decimates by 32) runs where N / decimate / 32 is at least 4 and a size this
 *     library has a transform for -- even, no prime factor beyond 7; where 32 does not divide the sizes they are truncated as
 *     create_filter_output truncates them (filter.c:103-107,116), the tone reading that much off, as in the reference;
 *   - FM channels need N / decimate <= 8192 (the post-detection filter lives in one CU's LDS).
 * Nothing limits max_channels but memory (~3 KiB per channel + the planes): banks of 34560 channels run in the bench. */
typedef struct kq_bank_config {
  int device;              /* HIP device ordinal.  A handle stays on its device: every call taking the handle runs
                            * there and restores the calling thread's current device, so one process can drive
                            * banks on several GPUs (kq_bank_create included). */
  int samprate;            /* front-end complex sample rate, Hz */
  unsigned L;              /* new samples per block            (demod->filter.L) */
  unsigned M;              /* impulse response length          (demod->filter.M); N = L+M-1: see Limits */
  unsigned decimate;       /* D: output rate = samprate / D    (demod->filter.decimate), >= 1 (1 -- a 48 kHz front end -- with
                              L + M - 1 <= 8192) */
  unsigned max_channels;
  unsigned max_blocks;     /* largest number of blocks one kq_bank_process call may take */
  float gain_factor;       /* demod->sdr.gain_factor (radio.c:122); 1.0 for synthetic float input */
  int compute_n0;          /* run the status-only compute_n0 (radio.c:383-425) every block */
  int fwd_mode;            /* enum kq_fwd_mode */
  void *stream;            /* hipStream_t to launch on, or NULL for the bank's own stream */
  int pl_tone_off;         /* 0 (default): pltask's PL / CTCSS tone measurement (fm.c:189-285) runs for every FM channel whenever
                            * its slave has a usable size (N/D >= 128), as every demod_fm of the reference starts it;
                            * 1: never (status.plfreq = NaN) -- SURVEY 8d measures the synthetic configs 2-5 without it */
} kq_bank_config;

/* One receiver channel: the fields of struct demod / struct modetab that the path reads
 * (radio.h:64-193, radio.h:35-50; defaults in modes.txt:25-39, main.c:113-117). */
typedef struct kq_channel_config {
  int demod_type;          /* enum kq_demod_type */
  int flat;                /* opt.flat : FM without de-emphasis filter and gain (fm.c:55, 164-172) */
  int isb;                 /* filter.isb : CROSS_CONJ slave (linear.c:78-79, filter.c:239-249) */
  int channels;            /* output.channels : 1 mono, 2 stereo (linear.c:291-300) */
  float low, high;         /* filter.low / filter.high, Hz */
  float kaiser_beta;       /* filter.kaiser_beta */
  float headroom;          /* agc.headroom, amplitude ratio (main.c:117: 10^(-15/20)) */
  float hangtime;          /* agc.hangtime, s */
  float recovery_rate;     /* agc.recovery_rate, dB/s */
  double second_lo;        /* set_second_LO() argument, Hz (radio.c:290-301); 0 freezes the NCO */
  double doppler;          /* set_doppler() arguments, Hz and Hz/s (radio.c:180-184) */
  double doppler_rate;
  double shift;            /* set_shift() argument, Hz (radio.c:304-311) */
  int pll;                 /* opt.pll : carrier-tracking PLL in linear mode (linear.c:129-246; modes CAM, AME, CISB) */
  int square;              /* opt.square : squaring loop for suppressed-carrier DSB / BPSK (mode DSB) */
} kq_channel_config;

/* Per channel, per block signal status: the demod->sig.* / agc.gain values the path produces
 * (radio.h:164-175), plus the integer decision state that must match the reference exactly. */
typedef struct kq_chan_status {
  float if_power;          /* radio.c:143-145 (halving accumulator, shared by all channels) */
  float bb_power;          /* fm.c:99, am.c:78, linear.c:302 */
  float n0;                /* smoothed noise density (fm.c:78-82, am.c:46-49); NaN when compute_n0 = 0 */
  float snr;               /* fm.c:102-103; NaN for linear without PLL (linear.c:309); 0 for AM */
  float foffset;           /* fm.c:148 */
  float pdeviation;        /* fm.c:153 */
  float agc_gain;          /* am.c / linear.c agc.gain after the block */
  float noise_gain;        /* filter.out->noise_gain (filter.c:472-497) */
  float plfreq;            /* fm.c:189-285 CTCSS (PL) tone estimate, Hz; NaN: none, not FM, or N/D < 128 */
  float cphase;            /* linear.c:219-223 carrier phase of the block, rad (PLL modes; else 0) */
  int32_t pll_lock;        /* linear.c:162-169 */
  int32_t lock_count;      /* linear.c:157-170 (sig.lock_timer) */
  int32_t squelch_count;   /* fm.c:70 snr_below_threshold after the block */
  int32_t hangcount;       /* am.c:26 / linear.c:33 hangcount after the block */
  int32_t blanked;         /* FM samples held at lastaudio this block (fm.c:141) */
  int32_t nout;            /* floats of audio this block: olen (mono) or 2*olen (stereo) */
} kq_chan_status;

/* The part of kq_chan_status a receiver reads with every block (kq_bank_pull_pcm_planes_compact_async): at real time the
 * 64-byte record is half of what a PCM delivery moves over the link, and most of it changes at the rate of the status
 * packets (radio_status.c), not of the blocks.  The whole record stays available through kq_bank_pull_status and the
 * full-plane pulls. */
typedef struct kq_chan_status_compact {
  float bb_power;          /* as kq_chan_status */
  float n0;
  float snr;
  float aux;               /* FM: foffset (fm.c:148); AM and linear: agc_gain (agc.gain after the block) */
  int32_t state;           /* FM: squelch_count (fm.c:70); AM and linear: hangcount */
  int32_t nout;            /* words of audio this block */
} kq_chan_status_compact;

/* Per-kernel device time accumulated since the last reset (HIP events on the bank's stream) */
typedef struct kq_timing {
  double filter_ms;        /* pre-detection filter kernel (mix + forward FFT + response + IFFT) */
  double demod_ms;         /* FM + AM + linear demodulator kernels */
  double ingest_ms;        /* format conversion + IF power */
  uint64_t filter_launches;
  uint64_t channel_blocks; /* channel-blocks processed by the filter kernel */
  double filter_max_ms;    /* the longest single filter INTERVAL of a call since the last reset (timing level 1: from the marker
                              queued in front of the call's filter kernels to the one behind them, as the device's queue
                              processed them).  It holds the kernels' run time, anything that kept the queue from starting them,
                              and the host's own delay between queueing the two markers: */
  double filter_max_submit_ms; /* ... the host's part of that longest interval: wall time between queueing its two markers.
                              Small (tens of microseconds) = the time went by on the device's side; about the interval = the
                              calling thread was off its core in the middle of the call */
  uint64_t filter_max_launch;  /* ... and which filter pass since the last reset it was (0-based; to find it in a kernel trace) */
} kq_timing;

const char *kq_last_error(void);
const char *kq_version(void);
/* The structs of this header carry no size fields; the library counts their revisions instead.  A host built against
 * this header checks kq_abi_version() == KQ_ABI_VERSION once at start-up: a mismatch means a struct (kq_bank_config,
 * kq_fanout_info ...) has gained a field since the host was compiled. */
#define KQ_ABI_VERSION 6
int kq_abi_version(void);
/* Number of visible HIP devices, or -1 when the HIP runtime cannot be initialised */
int kq_device_count(void);
/* Page-locked host memory for the streaming entry points (kq_bank_push_iq_async, kq_bank_pull_planes_async,
 * kq_bank_pull_pcm_planes_async): what a host would otherwise take from hipHostMalloc, so that a C, cgo or JNI host links
 * this library alone.  Usable with every device of the process.  NULL on failure (kq_last_error says why). */
void *kq_host_alloc(size_t bytes);
void kq_host_free(void *p);

/* --- lifetime --- */
kq_bank *kq_bank_create(const kq_bank_config *cfg);               /* main.c:232 create_filter_input */
int kq_bank_destroy(kq_bank *bank);                               /* filter.c:254 delete_filter_input */

/* --- channels: what set_mode() + the demod thread prologue do (radio.c:322-374; fm.c:27-67,
 *     am.c:21-41, linear.c:29-81): creates the slave, designs its response, arms the demodulator.
 *     Returns the channel index (>= 0) or -1. --- */
int kq_bank_add_channel(kq_bank *bank, const kq_channel_config *cfg);
/* n channels at once -- the same result as n calls of kq_bank_add_channel, but every distinct response is designed once
 * (one launch for all), every distinct compute_n0 mask is built once and every per-channel plane is uploaded with one copy:
 * a bank of tens of thousands of channels is set up in a second instead of a minute.  indices (may be NULL) receives the
 * channel numbers.  All or nothing: returns n, or -1 with no channel added.  Meant for set-up: its copies are immediate, so it
 * waits for the calls in flight first -- on a running bank kq_bank_add_channel per channel does not (0.02 ms of host time each). */
int kq_bank_add_channels(kq_bank *bank, const kq_channel_config *cfgs, unsigned n, int *indices);
/* The demodulator thread's epilogue once demod->terminate is set and it has been joined (fm.c:177-182, am.c:80,
 * linear.c:319: delete_filter_output on its slaves).  The other channels keep their numbers; the slot is a hole that
 * the next kq_bank_add_channel reuses (lowest hole first, with prologue state), and holes at the end are dropped.
 * The pre-detection filter launch still spans holes, so a bank with many long-lived ones is better rebuilt.
 * Every per-channel call on a removed channel fails with -1. */
int kq_bank_remove_channel(kq_bank *bank, int ch);
/* 1 when `ch` names a live channel, 0 for a hole or an index out of range */
int kq_bank_channel_active(const kq_bank *bank, int ch);
/* One past the highest live channel number (holes included) */
unsigned kq_bank_num_channels(const kq_bank *bank);
/* set_mode (radio.c:322-374) on a running channel: the demodulator is torn down and started afresh with the mode's
 * demod_type, flat, isb, channels, pll, square, recovery_rate, hangtime, low / high (swapped when low > high),
 * kaiser_beta, headroom and shift -- new slave and response, demodulator state back at its prologue values (AGC gain,
 * squelch, FM state, audio filter history, carrier loop).  What struct demod keeps survives: both input
 * oscillators keep running (second_lo / doppler of `mode` are ignored), the shift oscillator keeps its phase,
 * sig.n0, sig.foffset and sig.pdeviation keep their values.  (The reference then re-runs set_freq to pull the second
 * LO back into range, radio.c:370 -- control plane, left to the caller.) */
int kq_bank_set_mode(kq_bank *bank, int ch, const kq_channel_config *mode);

/* --- tuning, all phase continuous and effective from the next block (osc.c:22-36) ---
 * None of the calls of this section, nor kq_bank_add_channel / remove_channel / set_mode / set_filter / set_n0, waits for
 * the device: what they change gathers in pinned queues and the next kq_bank_process applies it on the device, behind the
 * calls already queued (which keep the values they were queued with) and in front of its own kernels -- a new filter
 * response included, which is designed on the bank's stream where it is used (kq_bank_get_response then fetches it).  A
 * bank running at real time with several calls in flight is not stalled by its control plane (0.001-0.05 ms of host time
 * per operation at 32768 channels; carrier-tracking channels included since round 6: a loop's slot is its own and is
 * started afresh by the queue.  Only kq_bank_get_response of a channel whose filter has just been set waits, and a
 * carrier-tracking channel that needs a new chunk of 64 slots allocated). */
/* demod->filter.isb and demod->output.channels of a running linear channel (linear.c:117-120, 291-300): the slave's
 * out_type and the mono / stereo hand-off change from the next block on; AGC state and response are left alone. */
int kq_bank_set_linear_options(kq_bank *bank, int ch, int isb, int channels);
/* Second LO and Doppler: the new setting mixes the samples pushed from now on; the M - 1 samples before them, the history of
 * the windows to come, keep what they were mixed with (radio.c:132-139 mixes sample by sample).  That holds for every block
 * the old samples reach into -- one where M - 1 <= L, two with the reference's default -L 3840 -M 4353, across calls if the
 * calls are short.  A channel may be set again while old samples of its previous settings are still inside its history
 * (M - 1 > L and a retune before every block): up to five transitions per window are kept apart; a sixth inside the same
 * M - 1 samples (only possible where M - 1 > 5 L) treats the oldest samples as mixed with the oscillator after theirs. */
int kq_bank_set_second_lo(kq_bank *bank, int ch, double hz);                 /* radio.c:290 set_second_LO */
int kq_bank_set_doppler(kq_bank *bank, int ch, double hz, double hz_per_s);  /* radio.c:180 set_doppler */
int kq_bank_set_shift(kq_bank *bank, int ch, double hz);                     /* radio.c:304 set_shift */
int kq_bank_set_filter(kq_bank *bank, int ch, float low_hz, float high_hz, float kaiser_beta); /* filter.c:500 set_filter */
/* demod->sig.n0 as the demodulator finds it when it starts: NaN = the first compute_n0 result is taken as it comes,
 * anything else = the smoothing goes on from there (fm.c:78-82, am.c:46-49, linear.c:123-126).  A fresh channel has NaN. */
int kq_bank_set_n0(kq_bank *bank, int ch, float n0);

/* --- data path --- */
/* Append nsamples complex samples of the given format to the bank's input ring.  `iq` is a host
 * pointer, or a device pointer when is_device != 0.  Conversion/scaling as radio.c:110-122. */
int kq_bank_push_iq(kq_bank *bank, const void *iq, size_t nsamples, int format, int is_device);
/* One front-end datagram exactly as `radio` takes it off the wire: RTP header incl. CSRCs, extension
 * and padding (multicast.c:242-277, main.c:318-328), payload type IQ_PT = 97 (int16 I/Q) or IQ_PT8 = 98 (int8 I/Q)
 * (multicast.h:19-20; anything else is ignored, main.c:329-330), the obsolete 24-byte status block skipped
 * (main.c:338-341, sdr.h:18-48), then proc_samples' bookkeeping (radio.c:62-104): rtp_process (multicast.c:305-340)
 * decides whether the packet is a duplicate / stale (dropped), in sequence, or ahead with a timestamp gap -- in which
 * case the lost samples are injected as zeros with the LOs kept running (kq_bank_push_zeros) before the payload is
 * converted and appended (kq_bank_push_iq).  Packets are taken in arrival order; the reference's small
 * sort-by-sequence queue (main.c:347-357) stays with the caller.
 * Returns the number of samples appended by this call (zeros + payload), 0 for an ignored or dropped datagram, -1 on
 * error, and -2 when the ring has no room right now: run kq_bank_process and hand the SAME datagram in again, until it
 * is taken --   while ((n = kq_bank_push_rtp(b, pkt, len)) == -2) kq_bank_process(b);
 * The ring holds max_blocks * L samples plus L - 1 of slack, so a partly filled block never stands in the way of a packet
 * that fits the ring as such.  With whole blocks waiting, -2 leaves sequence, timestamp and counters untouched.  With
 * none waiting the gap's zero fill (up to 192000 samples, radio.c:79-100) is itself larger than the ring: each call then
 * puts in as many zeros as fit and moves the timestamp past them before it returns -2, so every round brings the gap a
 * ring closer to its end, sample for sample as the reference fills it; the packet is counted once.  A payload larger
 * than the whole ring is an error (-1; its samples become a gap that the next packet fills with zeros).
 * The call does not wait for the device: payloads gather in pinned host memory and go to the ring as one asynchronous
 * copy + conversion per run of packets, queued by the next kq_bank_process (or by any other call that touches the ring);
 * kq_bank_blocks_ready counts them at once. */
int kq_bank_push_rtp(kq_bank *bank, const void *datagram, size_t size);
typedef struct kq_rtp_counters {   /* struct rtp_state (multicast.h:41-50) + demod->input.samples */
  uint32_t ssrc;
  uint16_t next_seq;
  uint32_t next_timestamp;
  int64_t packets, drops, dupes;
  int64_t samples;
} kq_rtp_counters;
int kq_bank_rtp_counters(const kq_bank *bank, kq_rtp_counters *out);
/* Lost-sample zero fill (radio.c:81-100): append `nsamples` zeros; LOs keep running. */
int kq_bank_push_zeros(kq_bank *bank, size_t nsamples);
/* Number of complete blocks waiting in the ring */
unsigned kq_bank_blocks_ready(const kq_bank *bank);
/* Run mix + filter + demod for up to max_blocks waiting blocks on every channel
 * (radio.c:140-146 execute_filter_input, then each demod thread's loop body).
 * Asynchronous on the bank's stream.  Returns the number of blocks processed, or -1. */
int kq_bank_process(kq_bank *bank);
/* Convenience for resident-input benchmarks: process `nblocks` blocks reading the window
 * [M-1 history | nblocks*L] straight from `iq_dev` (device, complex float), no ring copy. */
int kq_bank_process_resident(kq_bank *bank, const void *iq_dev, unsigned nblocks);
/* The part of the path that follows the master (what a demodulator thread of the reference does with
 * filter.in->fdomain): `spectrum_dev` = nblocks x N complex float bins in device memory, the master's forward
 * transform of each block (execute_filter_input, filter.c:151) -- execute_filter_output (filter.c:206-250),
 * compute_n0 (radio.c:383-425) and the demodulators run on it; nothing is mixed or transformed forward.  Channels must
 * have no second LO / Doppler set (that mix sits in front of the master, radio.c:132-139); status.if_power is left 0
 * (radio.c:143-145 belongs to whoever fed the master).  The demodulator thread entry points use this on the compat
 * master's resident spectrum. */
int kq_bank_process_spectrum(kq_bank *bank, const void *spectrum_dev, unsigned nblocks);
/* The demodulators of a call may run on a second internal stream, overlapping the next call's filter pass (the bank
 * decides per call: after kq_bank_pull_planes_async, or with AM / SSB channels; KQ_DEMOD_OVERLAP=0 / 1 forces it).
 * kq_bank_join makes the bank's main stream wait (on the device) for the last call's demodulators wherever they ran;
 * kq_bank_sync applies what the control plane has queued since the last call and blocks the host until everything
 * issued so far has finished. */
int kq_bank_join(kq_bank *bank);
int kq_bank_sync(kq_bank *bank);
/* The hipStream_t the bank launches on, as void*: kq_bank_config.stream, or the bank's own stream when that was NULL.
 * A C host without the HIP headers hands it to kq_fanout_acquire / kq_fanout_release as the consumer stream. */
void *kq_bank_stream(kq_bank *bank);

/* --- streaming host I/O ---
 * Both ends of the path are host buffers in the reference: a packet's samples in (radio.c:106-147), one float buffer
 * per block out (audio.c:82 send_mono_output(demod, samples, olen)).  These three move whole batches between PINNED host
 * memory (hipHostMalloc / hipHostRegister) and the bank on copy streams of their own, under the kernels of the
 * neighbouring calls; nothing here blocks the host but kq_bank_host_io_wait.
 *  kq_bank_push_iq_async:     kq_bank_push_iq from host memory without the wait: the samples travel on the input copy
 *                             stream into one of two staging buffers, the conversion kernel follows them on the bank's
 *                             stream.  `iq` must stay unchanged until kq_bank_host_io_wait or until two more pushes
 *                             have been queued.
 *  kq_bank_pull_planes_async: queues the copy of the last call's outputs -- audio [channels][max_blocks][2 * olen] float
 *                             (of each channel-block the first status.nout floats are written, the rest of its row is
 *                             left as it was) and status [channels][max_blocks] (either may be NULL) -- on the output copy stream;
 *                             the next call's demodulators wait for it on the device before they overwrite the planes.
 *  kq_bank_pull_pcm_planes_async: the same delivery in the reference's own output format (audio.c:22-28, 45-50, 95-100):
 *                             pcm [channels][max_blocks][2 * olen] clipped int16 in network byte order (status.nout words
 *                             per channel-block), silent_mask [channels][max_blocks] (may be NULL; bit i set: the i-th
 *                             480-word chunk is all zero, the packet send_mono_output would not send) and the status
 *                             plane -- half the bytes of the float plane; the conversion rides in the copy kernel and
 *                             does not need kq_bank_enable_pcm.  olen a multiple of 8.
 *  kq_bank_pull_pcm_planes_compact_async: the same with kq_chan_status_compact records (24 bytes per channel-block
 *                             instead of 64; the plane 16-byte aligned) -- a third fewer bytes per delivery at N/D = 64.
 *  kq_bank_pull_wait:         blocks until the delivery queued `lag` deliveries before the newest one has landed (0: the
 *                             newest; at most 7) -- a streaming host takes the planes of call k-2 in hand while calls
 *                             k-1 and k are in flight.
 *  kq_bank_host_io_wait:      blocks until every queued copy has landed.
 * Call order for full overlap: process batch k, push batch k+1, then pull the planes of batch k --
 *     push(0); for k: { process(); push(k + 1); pull_planes(k); }
 * an input copy queued behind an output copy may share its hardware queue and then waits with it for the demodulators. */
int kq_bank_push_iq_async(kq_bank *bank, const void *iq_pinned, size_t nsamples, int format);
int kq_bank_pull_planes_async(kq_bank *bank, float *audio_pinned, kq_chan_status *status_pinned);
int kq_bank_pull_pcm_planes_async(kq_bank *bank, int16_t *pcm_pinned, uint32_t *silent_mask_pinned, kq_chan_status *status_pinned);
int kq_bank_pull_pcm_planes_compact_async(kq_bank *bank, int16_t *pcm_pinned, uint32_t *silent_mask_pinned,
                                          kq_chan_status_compact *status_pinned);
int kq_bank_pull_wait(kq_bank *bank, unsigned lag);
int kq_bank_host_io_wait(kq_bank *bank);

/* --- results of the last kq_bank_process call (replace send_mono_output/send_stereo_output,
 *     audio.c:82 / audio.c:32, and the sig.* fields read by radio_status.c:170-203) --- */
unsigned kq_bank_olen(const kq_bank *bank);                       /* filter.c:116 */
unsigned kq_bank_last_blocks(const kq_bank *bank);
/* Audio of channel ch for block blk of the last call: status.nout floats. Synchronises. */
int kq_bank_pull_audio(kq_bank *bank, int ch, unsigned blk, float *dst, size_t cap, size_t *n);
int kq_bank_pull_status(kq_bank *bank, int ch, unsigned blk, kq_chan_status *st);
/* PCM output stage (audio.c:22-28 scaleclip, audio.c:45-50 / 95-100): once enabled, every process call
 * also converts the audio plane to clipped int16 in network byte order on the device.  kq_bank_pull_pcm returns the
 * status.nout words of one channel-block and a mask whose bit i is set when the i-th 480-word chunk is all zero --
 * send_mono_output / send_stereo_output skip such a packet but still advance the RTP timestamp (audio.c:101-104).
 * Geometries with more than 32 packets per block (2 * olen > 15360 words) are refused. */
int kq_bank_enable_pcm(kq_bank *bank, int on);
int kq_bank_pull_pcm(kq_bank *bank, int ch, unsigned blk, int16_t *dst_be, size_t cap_words, size_t *nwords,
                     uint32_t *silent_mask);
/* The datagrams send_mono_output / send_stereo_output (audio.c:32-132) would hand to send() for one channel-block,
 * built on the host from the PCM plane: RTP header (multicast.c:282-294; payload type PCM_MONO_PT = 11 or
 * PCM_STEREO_PT = 10, multicast.h:22-23), 480-word chunks, all-zero chunks skipped while the timestamp still
 * advances, marker bit on the first packet after silence, sequence numbers on sent packets only.  Packets are written
 * back to back as [2-byte little-endian length][bytes].  The per-channel state (demod->output.rtp, output.silent)
 * advances, so call it once per channel-block, in order.  Returns the number of packets, or -1. */
typedef struct kq_out_rtp_state {
  uint32_t ssrc;
  uint16_t seq;
  uint32_t timestamp;
  int32_t silent;
  int64_t packets, bytes;
} kq_out_rtp_state;
int kq_bank_set_output_ssrc(kq_bank *bank, int ch, uint32_t ssrc);
int kq_bank_pull_rtp_audio(kq_bank *bank, int ch, unsigned blk, unsigned char *dst, size_t cap, size_t *used);
/* The same datagrams built from planes the host already holds -- pcm [channels][max_blocks][2 * olen] and status
 * [channels][max_blocks] as kq_bank_pull_pcm_planes_async delivered them: host work only, no device access, no wait; the
 * per-channel RTP state advances exactly as with kq_bank_pull_rtp_audio (call it once per channel-block, in order; do
 * not mix the two on one channel-block).  Channels are independent: a host with tens of thousands of them spreads the
 * channel range over its threads. */
int kq_bank_rtp_from_planes(kq_bank *bank, int ch, unsigned blk, const int16_t *pcm_plane, const kq_chan_status *status_plane,
                            unsigned char *dst, size_t cap, size_t *used);
int kq_bank_output_rtp_state(const kq_bank *bank, int ch, kq_out_rtp_state *out);
/* Pre-detection filter output (filter.out->output.c, olen complex) before demodulation */
int kq_bank_pull_filter_output(kq_bank *bank, int ch, unsigned blk, float *dst_re_im, size_t cap_complex);
/* The PL slave's output of one FM channel-block of the last call (pltask's pl_filter->output.r, fm.c:234,239: PL_L =
 * floor(olen / 32) floats, what the tone tracker appends to its ring); *n = PL_L.  -1 with a text when the PL measurement is
 * off (pl_tone_off, or a geometry without a PL slave), the channel is not FM, or cap < PL_L. */
int kq_bank_pull_pl_samples(kq_bank *bank, int ch, unsigned blk, float *dst, size_t cap, size_t *n);
/* Master spectrum fdomain[N] of one channel/block (only in KQ_FWD_FULL mode; radio.c:396) */
int kq_bank_pull_spectrum(kq_bank *bank, int ch, unsigned blk, float *dst_re_im, size_t cap_complex);
/* Designed responses (filter.out->response, N/D complex; FM audio response N/D/2+1).  The pre-detection response of a
 * channel added or changed one at a time lives on the device (it is designed there, on the bank's stream): the first
 * kq_bank_get_response after such a change applies what is queued, waits for the device and fetches it. */
int kq_bank_get_response(kq_bank *bank, int ch, float *dst_re_im, size_t cap_complex);
int kq_bank_get_audio_response(kq_bank *bank, int ch, float *dst_re_im, size_t cap_complex);
/* Device-resident result planes for zero-copy consumers:
 *   audio  : float [max_channels][max_blocks][2*olen]
 *   status : kq_chan_status [max_channels][max_blocks] */
void *kq_bank_audio_device_ptr(kq_bank *bank);
void *kq_bank_status_device_ptr(kq_bank *bank);

/* --- measurement --- */
/* on = 0: off; 1: HIP events around the filter kernel only (two stream operations per call); 2: around the ingest /
 * IF-power and demodulator kernels as well */
int kq_bank_enable_timing(kq_bank *bank, int on);
int kq_bank_get_timing(kq_bank *bank, kq_timing *t, int reset);
/* The HOST's own time inside kq_bank_process / _resident / _spectrum since the last reset -- what scales with the number of
 * channels on the host side of a call (the kernels are only queued there).  A receiver at 1.0 x real time with tens of
 * thousands of channels and a batch of a few blocks has about a millisecond per call: this is the figure to watch.
 * No reference analogue (each `radio` process steps its own oscillators per sample, radio.c:132-136). */
typedef struct kq_host_timing {
  double call_ms;          /* wall time inside the process calls, everything included */
  double stage_ms;         /* of that: evaluating and staging the per-channel oscillator parameters of the call */
  double slot_wait_ms;     /* of that: blocked because the device was four calls behind (back-pressure, not work); taken
                              with the handle's lock let go, so control-plane calls from another thread run meanwhile */
  uint64_t calls;
  /* The handle's lock between the receiver thread (the process calls) and whoever drives the control plane (set_* / add /
   * remove from another thread; main.c's UI and status threads beside proc_samples): */
  double lock_wait_ms;     /* total the process calls waited to get the lock (not part of call_ms) */
  double lock_wait_max_ms; /* the worst single wait: what a control-plane call cost the stream at most */
  double ctl_hold_max_ms;  /* the longest any OTHER entry point held the lock (device waits with the lock let go excluded) */
} kq_host_timing;
int kq_bank_get_host_timing(kq_bank *bank, kq_host_timing *t, int reset);
/* The entry point behind ctl_hold_max_ms (its name, e.g. "kq_bank_set_filter"; "" when nothing has held the lock since the
 * last reset).  Read it before the kq_bank_get_host_timing call that resets. */
const char *kq_bank_worst_lock_holder(kq_bank *bank);
/* Which forward path the bank resolved to (enum kq_fwd_mode, never AUTO) */
int kq_bank_fwd_mode(const kq_bank *bank);

/* ---- multi-GPU: channel shards and the front-end fan-out ------------------------------------------------------------
 * The reference runs one `radio` process per channel and fans the front-end I/Q stream out to them by UDP multicast
 * (multicast.c:143-237, README.md:470-477).  Here one process (or thread) per GPU owns a contiguous range of the
 * channels and every batch of front-end samples is broadcast from the ingest rank over RCCL / xGMI (ncclBroadcast on a
 * side stream, two slots so that batch k+1 travels while batch k is processed).  Channels are independent: this is
 * the only exchange on the path.  librccl is loaded on first use.
 *
 *   rank `root`:  kq_fanout_unique_id(id)  -> hand the 128 bytes to the other ranks (file, socket, MPI ...)
 *   every rank:   f = kq_fanout_create(device, rank, world, root, id, samples_per_batch);
 *                 COLLECTIVE: ncclCommInitRank inside returns only once all `world` ranks have called it with the same
 *                 id -- one thread or process per rank, all calling concurrently (one thread creating the fan-outs of
 *                 several ranks one after the other would wait on itself for ever).  A rank whose own set-up fails
 *                 (memory, stream) still enters the communicator, and the ranks then agree through a one-word
 *                 ncclAllReduce, issued by every rank that holds a communicator whatever else went wrong on it: either
 *                 every rank gets its fan-out or every rank gets NULL (kq_last_error says which side it was on).
 *                 What this cannot cover: ncclCommInitRank itself failing, or librccl missing, on a SUBSET of the ranks --
 *                 the others then wait inside RCCL, and only the caller's own timeout ends that.
 *                 KQ_RCCL_LIB in the environment names the librccl to dlopen.
 *                 kq_shard_range(total_channels, world, rank, &first, &count) -> add channels first .. first+count-1
 *   per batch k:  slot = k & 1
 *                 kq_fanout_post(f, slot, iq, n, is_device)      queue the broadcast (iq: read on the root rank only)
 *                 p = kq_fanout_acquire(f, slot, bank_stream, &n)                  bank_stream waits for the batch
 *                 kq_bank_process_resident(bank, p, nblocks)                       (window layout: M-1 history + blocks)
 *                 kq_fanout_release(f, slot, bank_stream)                          the slot may be overwritten after this
 * `bank_stream` is the hipStream_t the bank was created on (kq_bank_config.stream); it must outlive the fan-out's next
 * kq_fanout_post of that slot (a world of one without a communicator records the release on it only then, and only if
 * that post copies something into the slot). */
#define KQ_FANOUT_ID_BYTES 128
typedef struct kq_fanout kq_fanout;
/* contiguous, balanced range of `rank`: the first total % world ranks hold one channel more */
int kq_shard_range(unsigned total, unsigned world, unsigned rank, unsigned *first, unsigned *count);
int kq_fanout_unique_id(void *id128);
kq_fanout *kq_fanout_create(int device, int rank, int world, int root, const void *id128, size_t max_samples);
int kq_fanout_destroy(kq_fanout *f);
int kq_fanout_post(kq_fanout *f, int slot, const void *iq_cf32, size_t nsamples, int src_is_device);
const void *kq_fanout_acquire(kq_fanout *f, int slot, void *consumer_stream, size_t *nsamples);
int kq_fanout_release(kq_fanout *f, int slot, void *consumer_stream);
/* what the fan-out has done so far: the world as RCCL itself counts it (ncclCommCount; 0 without a communicator), the
 * library's version code (ncclGetVersion) and the time the broadcasts took on the side stream (HIP events around
 * ncclBroadcast; a broadcast still in flight when its slot was posted again is not counted).  Waits for the side stream. */
typedef struct kq_fanout_info {
  int world, rank;
  int rccl_ranks, rccl_version;
  unsigned long long broadcasts;
  double broadcast_ms;
  /* consumer side: kq_fanout_acquire calls so far; of those, the ones that found their batch not yet landed while
   * kq_fanout_enable_timing was on (`waits`), and the time the consumer stream then stood still for it (`wait_ms`, HIP
   * events on that stream around the wait: a stalled step shows here, a slow broadcast that still arrives in time does not) */
  unsigned long long acquires, waits;
  double wait_ms;
  /* acquires that had to wait but went untimed because the slot's previous timed wait was still in flight (the host several
   * steps ahead of a stalled device): wait_ms / waits describe the timed ones only */
  unsigned long long waits_dropped;
} kq_fanout_info;
int kq_fanout_stats(kq_fanout *f, kq_fanout_info *out);
/* Path of the shared object ncclBroadcast was bound from (dladdr), "" before librccl has been loaded or when it could not
 * be: a process that also holds torch has torch's own copy of librccl mapped, and the dynamic loader hands this library
 * whichever `librccl.so.1` it finds first -- one line of a bench or log says which one carried the broadcasts. */
const char *kq_fanout_rccl_path(void);
/* on != 0: time the consumer's waits (two event records on the consumer stream per acquire that has to wait, ~5 us each
 * behind a long kernel -- a diagnostic, off by default). */
int kq_fanout_enable_timing(kq_fanout *f, int on);

/* --- front-end half-band decimator cascade ---------------------------------------------------
 * What hackrf.c:260-330 does to every block of raw A/D samples before they reach the channel filter: rotate by
 * +offset*Fs/4 (hackrf.c:272-291), run log_decimate half-band stages -- hb3_block (decimate.c:146-160) while the
 * stage index j >= stage_threshold, hb15_block (decimate.c:108-144) below it (hackrf.c:295-300) -- multiply by
 * Filter_atten (hackrf.c:469), convert to int16 (hackrf.c:307-311) and sum the output energy.  The filter state
 * (struct hb15_state / hb3state, hackrf.c:211-216) is carried inside the handle across calls. */
typedef struct kq_decimator kq_decimator;
typedef struct kq_decim_config {
  int device;
  int log_decimate;     /* hackrf.c:64 Log_decimate: decimation ratio is 2^log_decimate */
  int stage_threshold;  /* hackrf.c:76: stages j >= this use the 1-2-1 filter */
  int offset;           /* hackrf.c:68 Offset: rotate_phase increment per input sample, 0 = no rotation */
  float filter_atten;   /* hackrf.c:65,469 Filter_atten; 0 selects 0.5^log_decimate */
  size_t max_out;       /* largest n_out of one process call */
  void *stream;         /* hipStream_t to run on, NULL = private stream */
} kq_decim_config;
kq_decimator *kq_decim_create(const kq_decim_config *cfg);
int kq_decim_destroy(kq_decimator *d);
/* hb15 coefficients, order as struct hb15_state.coeffs (decimate.h:5); default is hackrf.c:229-238 */
int kq_decim_set_coeffs(kq_decimator *d, const float coeffs[4]);
/* iq_in: n_out << log_decimate interleaved complex float samples.  out_cf32: n_out complex samples after
 * Filter_atten; out_s16 (may be NULL): the same as (short)round(32767*s), interleaved I,Q; out_energy (may be
 * NULL): sum of s*s over the call (hackrf.c:308,325 output_energy), added up inside the last kernel of the call in an
 * order fixed by the device (same input, same device: same bits).  on_device != 0: every pointer is device
 * memory and the call is asynchronous on the handle's stream; otherwise host memory, synchronous.
 * kq_decim_sync (and a host-memory call) returns -1 if a workgroup's share of the energy never arrived (a device fault;
 * that call's energy is NaN, its samples are unaffected). */
int kq_decim_process(kq_decimator *d, const float *iq_in, int on_device, size_t n_out, float *out_cf32,
                     int16_t *out_s16, float *out_energy);
int kq_decim_sync(kq_decimator *d);
int kq_decim_reset(kq_decimator *d);

/* --- raw A/D conditioning ahead of the cascade -----------------------------------------------------------------
 * What the front-end daemons do to every sample that comes off the A/D before the Fs/4 rotation and the cascade
 * (hackrf.c:122-196 rx_callback, funcube.c:287-390): integer to float, DC removal, I/Q gain balance at constant total
 * energy, I/Q phase correction, and the running estimates behind them, updated once per block.
 *
 * Definition.  The stream is cut into blocks of `block` samples, counted from the first sample after create / reset,
 * whatever the call boundaries are.  For int8 a raw -128 counts one clip and becomes -127 (hackrf.c:146-153).  With the
 * float constants DC_i, DC_q, gain_i, gain_q, secphi, tanphi in force at the start of a sample's block, per sample, in
 * float, unfused, in the reference's operand order:
 *     x = float(i) * SCALE - DC_i;  y = float(q) * SCALE - DC_q;  x *= gain_i;  y *= gain_q;  y = secphi * y - tanphi * x
 * SCALE = (float)(1./127) for int8, (float)(1./32767) for int16.  Output cf32 is (x, y); output int16 is
 * round(v * 32767) (funcube.c:348), saturated to +-32767 ... -32768.
 * Per block, in double (+ - * / sqrt, no fused operations), from the exact integer moments n = block, SI, SQ, SII, SQQ,
 * SIQ of the block's samples, S = (double)SCALE and the constants above:
 *     sum_i = S * SI;  sum_q = S * SQ
 *     i_energy = S * S * SII - 2 * DC_i * (S * SI) + n * (DC_i * DC_i)           (q_energy alike)
 *     dotprod  = (gain_i * gain_q) * (S * S * SIQ - DC_q * (S * SI) - DC_i * (S * SQ) + n * (DC_i * DC_q))
 * then the reference's update (hackrf.c:182-193), every stored value rounded to float:
 *     DC_i += dc_alpha * (sum_i - n * DC_i)                                       (DC_q alike, with the old DC)
 *     block_energy = 0.5 * (i_energy + q_energy);  only if block_energy > 0:
 *       in_power = block_energy / n
 *       imbalance += r * (i_energy / q_energy - imbalance)      r = block / (adc_samprate * power_alpha)
 *       sinphi    += r * (dotprod / block_energy - sinphi)
 *       gain_q = sqrt(0.5 * (1 + imbalance));  gain_i = sqrt(0.5 * (1 + 1 / imbalance))
 *       secphi = 1 / sqrt(1 - sinphi * sinphi);  tanphi = sinphi * secphi
 * Initial state: DC = 0, imbalance = 1, sinphi = 0, in_power = 0, gains and secphi 1, tanphi = 0.  The integer sums do
 * not depend on the order they are formed in, so the result is the same bits on every device and for every way of cutting
 * the stream into calls; it differs from the reference's literal loop by that loop's own float rounding of its sums
 * (DESIGN 4.14).  A partial block at the end of a call leaves its moments and clip count in the handle.
 *
 * Calls: kq_fe_create checks its arguments before it touches a device.  on_device != 0: every pointer is device memory
 * (raw 16-byte aligned) and the call is asynchronous on the handle's stream; otherwise host memory, synchronous.  There is
 * no CPU path. */
typedef struct kq_frontend kq_frontend;
enum kq_fe_format { KQ_FE_S8 = 0, KQ_FE_S16 = 1 }; /* interleaved I,Q: int8 (HackRF) or int16 in host byte order (Funcube) */
typedef struct kq_fe_config {
  int device;
  int format;          /* enum kq_fe_format */
  unsigned block;      /* samples per update, 64 .. 1 << 22 (the int16 second moments then stay below 2^53) */
  double adc_samprate; /* > 0 */
  double dc_alpha;     /* > 0, per sample: hackrf.c:74 has 1e-7, funcube.c:65 1e-6 */
  double power_alpha;  /* > 0, seconds: hackrf.c:75, funcube.c:66 have 1.0 */
  size_t max_samples;  /* largest n of one call (n_out << log_decimate for kq_fe_process_decim) */
  void *stream;        /* hipStream_t to run on, NULL = private stream */
} kq_fe_config;
/* The state after a completed block. */
typedef struct kq_fe_status {
  unsigned long long samples; /* samples in completed blocks since create / reset */
  unsigned long long blocks;
  unsigned long long clips;   /* int8 -128 values met in completed blocks, I and Q counted separately */
  float DC_i, DC_q, imbalance, sinphi, in_power;
  float gain_i, gain_q, secphi, tanphi; /* in force from the next block on */
  float reserved_;
} kq_fe_status;
kq_frontend *kq_fe_create(const kq_fe_config *cfg);
int kq_fe_destroy(kq_frontend *fe);
int kq_fe_reset(kq_frontend *fe);
int kq_fe_sync(kq_frontend *fe);
void *kq_fe_stream(kq_frontend *fe); /* the hipStream_t the handle runs on, for a kq_decim_config / kq_bank_config beside it */
/* Conditions n samples (any n up to max_samples).  raw: n I,Q pairs of the configured format.  out_cf32 (n complex
 * floats) and out_s16 (n I,Q int16 pairs) may each be NULL.  block_status (may be NULL) receives one record for each block
 * completed inside the call, in order: at most (n + block - 1) / block of them; the return value is their number, -1 on
 * error. */
int kq_fe_process(kq_frontend *fe, const void *raw, int on_device, size_t n, float *out_cf32, int16_t *out_s16,
                  kq_fe_status *block_status);
/* Conditions n_out << log_decimate raw samples and runs dec's cascade on them; out_cf32, out_s16, out_energy as for
 * kq_decim_process.  Outputs and the carried state of both handles are those of kq_fe_process into a buffer followed by
 * kq_decim_process on that buffer, but no input-rate float buffer is written: the cascade's first kernel reads the raw
 * samples.  fe and dec must be on the same device and stream. */
int kq_fe_process_decim(kq_frontend *fe, kq_decimator *dec, const void *raw, int on_device, size_t n_out, float *out_cf32,
                        int16_t *out_s16, float *out_energy, kq_fe_status *block_status);
/* The state after the last completed block; waits for the handle's stream. */
int kq_fe_get_status(kq_frontend *fe, kq_fe_status *out);

/* --- AFSK-1200 / HDLC packet decoder -----------------------------------------------------------
 * What the `packet` program does per RTP session between its PCM input and a decoded AX.25 frame: the REAL master
 * filter of 1000 new samples / 1049 taps (packet.c:41-45,190), the analytic 100..4000 Hz slave (packet.c:272-273),
 * the mark / space correlators with on-time and mid-bit integrators, the Gardner-style bit clock, NRZI and HDLC
 * deframing (packet.c:276-410) and the frame check (ax25.c:138-156 crc_good).  Constants are the reference's: 48 kHz
 * audio, 1200 bit/s, 40 samples per bit.  A bank holds `max_sessions` independent sessions that advance in lock step;
 * decoded frames (body + the two FCS bytes, exactly what packet.c:356 sends) collect in a per-session arena. */
typedef struct kq_afsk_bank kq_afsk_bank;
enum kq_pcm_format {
  KQ_PCM_F32 = 0,   /* float samples, what packet.c:207 stores into input.r[] */
  KQ_PCM_S16BE = 1, /* 16-bit big-endian PCM words as they arrive in the RTP payload, converted as packet.c:207 does:
                       ntohs() is unsigned, so a negative word w becomes (w + 65536) / 32768 (quirk kept) */
  KQ_PCM_S16 = 2    /* int16 in host byte order scaled by 1/SHRT_MAX (modulate.c:24,136-141); kq_mod_process only */
};
typedef struct kq_afsk_config {
  int device;
  unsigned max_sessions;
  unsigned max_frames;   /* arena slots per session between kq_afsk_clear_frames calls */
  void *stream;          /* hipStream_t, NULL = private stream */
} kq_afsk_config;
typedef struct kq_afsk_state {   /* packet.c:286-299 after the last processed block */
  int symphase, frame_bit, flagsync, ones;
  float last_val, mid_val;
  int decoded_packets;           /* packet.c:34 */
  int pending_samples;           /* packet.c:31 input_pointer */
  uint64_t blocks;
} kq_afsk_state;
kq_afsk_bank *kq_afsk_create(const kq_afsk_config *cfg);
int kq_afsk_destroy(kq_afsk_bank *bank);
/* Append `nsamples` samples to every session (session i at samples + i * session_stride elements) and decode every
 * block of 1000 that completes (packet.c:204-211).  Returns the number of blocks decoded per session, or -1.
 * on_device != 0: `samples` is device memory and the call is asynchronous on the bank's stream. */
int kq_afsk_push(kq_afsk_bank *bank, const void *samples, int format, unsigned nsessions, size_t nsamples,
                 size_t session_stride, int on_device);
int kq_afsk_sync(kq_afsk_bank *bank);
int kq_afsk_num_frames(kq_afsk_bank *bank, unsigned session);
int kq_afsk_dropped_frames(kq_afsk_bank *bank, unsigned session);   /* good frames lost to a full arena */
/* Copies frame `index` of `session` (at most cap bytes) and returns its length (<= 1024), or -1 */
int kq_afsk_pull_frame(kq_afsk_bank *bank, unsigned session, unsigned index, unsigned char *dst, size_t cap);
int kq_afsk_clear_frames(kq_afsk_bank *bank);
/* filter.out->output.c of the last decoded block (1000 complex) and the decoder state, for parity checks */
int kq_afsk_pull_filter_output(kq_afsk_bank *bank, unsigned session, float *dst_re_im, size_t cap_complex);
int kq_afsk_pull_state(kq_afsk_bank *bank, unsigned session, kq_afsk_state *out);

/* --- modulator bank: many stations summed into one wideband I/Q stream ---------------------------------------------
 * modulate.c for thousands of stations at once.  Each station is one modulate.c instance with the zero-stuffing factor 4
 * generalised to `interp`: per block of L output samples it takes L / interp audio samples, zero-stuffs them into the REAL
 * input of an overlap-save filter (modulate.c:136-145) whose response is gain interp / N between `low` and `high`
 * (modulate.c:113-128, f evaluated in float) shaped by window_filter(L, M, response, kaiser_beta) (modulate.c:130), takes the
 * COMPLEX output at decimate 1 (modulate.c:131-132, filter.c:206-216), adds `carrier` (modulate.c:149-153) and multiplies by
 * step_osc(&osc) * amplitude (modulate.c:155-157).  The bank outputs the sum of its active stations, added in slot order
 * in a fixed tree (same calls, same bits; one block per call or max_blocks per call, same bits).
 * KQ_MOD_FM goes beyond the reference: m[n] = real part of the filter output, theta[n] = theta[n-1] + 2 pi deviation / Fs
 * m[n] (carried across blocks in double, wrapped at block boundaries, 0 when a station is added or turns to FM), baseband
 * exp(i theta[n]); `carrier` is ignored.
 * Deviation from the reference: int16 output is trunc(x * 32767) as modulate.c:160-163 but saturates outside the int16
 * range, where the reference's float-to-short conversion is undefined.
 * Limits: N = L + M - 1 even and 2^a 3^b 5^c 7^d up to 16384; interp >= 1 dividing L and M - 1; up to 65536 stations.
 * Stations with equal (low, high, kaiser_beta) share one designed response. */
typedef struct kq_mod_bank kq_mod_bank;
enum kq_mod_type {
  KQ_MOD_LINEAR = 0,  /* modulate.c:70-94: AM / USB / LSB / AME by the edges and the carrier */
  KQ_MOD_FM = 1       /* frequency modulation of the filtered audio (not in the reference) */
};
typedef struct kq_mod_config {
  int device;
  int samprate;             /* modulate.c:26 Samprate: output rate Fs; the audio rate is Fs / interp */
  unsigned L, M;            /* modulate.c:111-112: new samples per block, impulse length (N = L + M - 1, modulate.c:113) */
  unsigned interp;          /* modulate.c:136-145: zero-stuffing factor (4 there) */
  unsigned max_stations;    /* slots 0 .. max_stations - 1 */
  unsigned max_blocks;      /* largest nblocks of one kq_mod_process call */
  void *stream;             /* hipStream_t to run on, NULL = private stream */
} kq_mod_config;
typedef struct kq_station_config {
  int mod_type;             /* enum kq_mod_type */
  float low, high;          /* modulate.c:70-94: passband edges in Hz (AM -5000..5000, USB 0..3000, LSB -3000..0, AME 0..3000) */
  float carrier;            /* modulate.c:72,86: added to every filter output sample (0 or 1; linear only) */
  float kaiser_beta;        /* modulate.c:130: window_filter's beta, 3.0 there */
  float deviation;          /* FM peak deviation in Hz per unit of filtered audio */
  double frequency;         /* modulate.c:43,104: carrier frequency in Hz (set_osc's f * Fs, osc.c:22) */
  double sweep;             /* modulate.c:45,106: Hz per second (set_osc's r * Fs^2, osc.c:22) */
  double amplitude_dbfs;    /* modulate.c:44,105: amplitude = 10^(dBFS / 20) */
} kq_station_config;
/* NULL on failure; the configuration is checked before any HIP call.
 * Control plane: kq_mod_set_station, kq_mod_remove_station and kq_mod_reset are synchronous -- each waits for the bank's
 * stream, so for every kq_mod_process still queued there, before it returns (a new (low, high, kaiser_beta) also waits
 * for its response design).  Set stations up before the stream is busy; only kq_mod_process is asynchronous. */
kq_mod_bank *kq_mod_create(const kq_mod_config *cfg);
int kq_mod_destroy(kq_mod_bank *bank);
/* Add a station to an empty slot or change one.  A new station starts cold at the next call's first block (zero filter
 * history as filter.c:76, phasor 1); changing frequency, sweep or amplitude keeps the phase as set_osc does (osc.c:24-27);
 * changing the mode, the edges or beta swaps the response from the next block and keeps the history. */
int kq_mod_set_station(kq_mod_bank *bank, unsigned slot, const kq_station_config *station);
/* The station stops contributing from the next block */
int kq_mod_remove_station(kq_mod_bank *bank, unsigned slot);
/* Synthesise nblocks * L output samples.  pcm: station `slot`'s audio at pcm + slot * stride elements, nblocks * L / interp
 * samples each, in pcm_format KQ_PCM_F32 or KQ_PCM_S16; rows of empty slots are ignored, but host memory is read for
 * every row 0 .. the highest occupied slot, so the buffer must hold that many rows.  out_cf32 (nblocks * L interleaved complex floats) and out_s16 (nblocks * L interleaved
 * I,Q int16) may each be NULL, not both.  on_device != 0: every pointer is device memory and the call is asynchronous on the
 * bank's stream; otherwise host memory, synchronous. */
int kq_mod_process(kq_mod_bank *bank, const void *pcm, int pcm_format, size_t stride, unsigned nblocks, int on_device,
                   float *out_cf32, int16_t *out_s16);
int kq_mod_sync(kq_mod_bank *bank);
/* Every station restarts cold (history, oscillator and FM phase), keeping its settings */
int kq_mod_reset(kq_mod_bank *bank);

/* --- spectrum bank: averaged power spectra of the I/Q stream --------------------------------------------------------
 * Many analyzers over one wideband I/Q stream, each a view an operator places channels by: an overview of the whole
 * band or a zoom on part of it, optionally following a Doppler sweep.  Per analyzer and input sample x[n] (n counted from
 * create or kq_spec_reset across calls, x[n] = 0 for n < 0; s16 / s8 scaled as kq_bank_push_iq does, radio.c:110-122):
 *   mix       m[n] = x[n] exp(-2 pi i phi(n) / 2^64), phi(n) = inc n + inc2 d (d - 1) / 2 in uint64 arithmetic, d = n - s0
 *             (s0 = the stream index where the analyzer was set), inc = round(center / Fs 2^64), inc2 = round(sweep / Fs^2 2^64);
 *             exact, so the views do not drift and do not depend on how the stream is split into calls
 *   decimate  Dz = 1: y[j] = m[s0 + j].  Dz > 1: y[j] = sum_t h[t] m[s0 + j Dz - t], Lh = 24 Dz + 1 taps of a Kaiser (3.0)
 *             windowed sinc, cut-off at the decimated Nyquist, sum h = 1; the input history makes a new analyzer start clean
 *   frames    frame f = y[f H .. f H + Nf - 1] times w = make_kaiser(Nf, kaiser_beta) (filter.c:337-357), Nf-point transform,
 *             P_f[k] = |X_f[k]|^2 / (sum w)^2
 *   rows      row r = (1/K) sum of frames r K .. r K + K - 1 of P_f[k] / C[k] for k = -B/2 .. B/2 - 1 (row element 0 is the
 *             lowest frequency); C[k] = |H(k / (Dz Nf))|^2 undoes the decimator's passband shape (1 when Dz = 1).
 * Readings: a tone A e^{i w n} on a bin centre reads A^2; white noise of density N0 reads N0 enbw_bins bin_bw.
 * Frames are added in frame order with the accumulator carried across calls: the same input split differently gives the
 * same bits.
 * Device memory per analyzer: about (Nf + max_samples / Dz) 8 + B 4 (max_rows + 1) bytes, plus the frame powers of one call
 * (at most 2^21 floats; longer calls run in rounds), plus one bank-wide input history of 2 (6144 + max_samples) 8 bytes.
 * kq_spec_create touches no device: its checks need no GPU, and device memory is allocated by the first kq_spec_set.
 * Calls: kq_spec_process with device memory (on_device != 0) is asynchronous on the handle's stream and reads nothing back;
 * with host memory it is synchronous.  kq_spec_set, kq_spec_remove, kq_spec_reset and kq_spec_pull wait for the stream;
 * kq_spec_get_info answers from the host's account of the calls without waiting.  A change takes effect at the first sample of the next kq_spec_process.  One lock per handle: an operator
 * thread may set and remove analyzers while another thread processes and pulls. */
typedef struct kq_spec_bank kq_spec_bank;
typedef struct kq_spec_config {
  int device;
  int samprate;              /* Fs of the I/Q stream */
  float gain_factor;         /* demod->sdr.gain_factor, applied to every format as kq_bank_push_iq does (radio.c:122) */
  unsigned max_specs;        /* analyzer slots 0 .. max_specs - 1 (limit 4096) */
  size_t max_samples;        /* largest nsamples of one kq_spec_process call */
  unsigned max_rows;         /* output rows buffered per analyzer before new ones are dropped (and counted) */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_spec_config;
typedef struct kq_spec_params {
  double center;             /* Hz relative to the stream's centre, |center| <= samprate / 2 */
  double sweep;              /* Hz/s: the centre moves from the analyzer's start (Doppler-following views) */
  unsigned decimate;         /* Dz, 1..256 */
  unsigned fft_size;         /* Nf, even 2^a 3^b 5^c 7^d, 16..16384 */
  unsigned bins;             /* B, even; <= Nf when Dz = 1, <= 3 Nf / 4 when Dz > 1 */
  unsigned hop;              /* H, 1..Nf decimated samples between frames (Nf / 2 = 50 % overlap) */
  unsigned average;          /* K frames per output row, >= 1 */
  float kaiser_beta;         /* frame window, make_kaiser convention (filter.c:337-357), >= 0 */
} kq_spec_params;
typedef struct kq_spec_row {
  uint64_t start_sample;     /* s0 + r K H Dz: the stream index of the row's first frame's first decimated sample */
  uint32_t frames;           /* K */
  uint32_t generation;       /* the kq_spec_set that made the parameters of this row (1 for the first) */
} kq_spec_row;
typedef struct kq_spec_info {
  double bin_bw;             /* Fs / (Dz Nf) */
  double first_bin_hz;       /* centre of row element 0 at the analyzer's start: center - B / 2 bin_bw */
  double enbw_bins;          /* Nf sum w^2 / (sum w)^2 */
  double delay_samples;      /* the decimator's group delay in input samples: 12 Dz (0 when Dz = 1) */
  uint64_t rows_ready, rows_dropped;
  uint32_t frames_pending;   /* frames in the row being averaged */
  uint32_t generation;
} kq_spec_info;

kq_spec_bank *kq_spec_create(const kq_spec_config *cfg);
int kq_spec_destroy(kq_spec_bank *bank);
/* Add an analyzer to `slot` or replace the one there (generation + 1).  It starts at the next call's first sample with an
 * empty average; unpulled rows of the slot stay (with their old generation) unless B changes, then they count as dropped. */
int kq_spec_set(kq_spec_bank *bank, unsigned slot, const kq_spec_params *params);
/* The analyzer stops from the next call; its unpulled rows are discarded */
int kq_spec_remove(kq_spec_bank *bank, unsigned slot);
/* nsamples (0 .. max_samples) I/Q samples in `format` (enum kq_iq_format) */
int kq_spec_process(kq_spec_bank *bank, const void *iq, int format, size_t nsamples, int on_device);
/* Copy up to max_rows of the slot's oldest rows (B floats each) to host `rows` and, when meta is not NULL, their kq_spec_row;
 * returns the number copied */
int kq_spec_pull(kq_spec_bank *bank, unsigned slot, float *rows, unsigned max_rows, kq_spec_row *meta);
int kq_spec_get_info(kq_spec_bank *bank, unsigned slot, kq_spec_info *out);
int kq_spec_sync(kq_spec_bank *bank);
/* Stream index back to 0, input history zeroed, every analyzer restarts with its settings; unpulled rows are discarded */
int kq_spec_reset(kq_spec_bank *bank);

/* --- wideband FM stereo decoder bank ---------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each turning one broadcast FM composite ("stereo multiplex") into left and right audio.  The
 * composite is the unfiltered discriminator output of a flat FM channel (kq_channel_config.flat = 1) in rad/sample at
 * Fc = comp_rate; a receiver bank's audio plane (kq_bank_audio_device_ptr) can be decoded in place on its stream, after
 * kq_bank_join(bank) (the bank may write that plane from a second stream: see kq_bank_join).
 * The reference has no stereo decoder: the algorithm is defined here.
 * Geometry: Da = decimate, Fo = Fc / Da, frames of L new samples, filter length M (odd), N = L + M - 1, D = (M - 1) / 2.
 * Per slot, x[n] is the composite; n counts samples since create or kq_wfm_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.
 *   responses  each an ideal response sampled on the N bins, shaped by window_filter's procedure (filter.c:365-413: inverse
 *              transform, centre moved to M/2, make_kaiser(M, kaiser_beta), zero pad, forward transform) in double and used
 *              as float; both delay by D.  h_m (mono/audio): 1 for |f| <= 15 kHz times the de-emphasis 1 / (1 + j 2 pi f
 *              tau), tau = deemph_us (0 = none), Hermitian (real taps), one per distinct tau.  h_p (pilot, one-sided):
 *              1 for |f - 19000| <= pilot_bw / 2.
 *   pilot      p[n] = (h_p * x)[n], u[n] = p[n] / |p[n]| (0 where |p| = 0) ~ exp(j theta(n - D))
 *   difference d[n] = 2 x[n - D] Re(u[n]^2)
 *   sum, diff  a[n] = (h_m * x)[n - D], s[n] = (h_m * d)[n]: both delayed by 2 D
 *   output     j-th output at n = j Da: L_j = g (a + sigma s), R_j = g (a - sigma s), g = Fc / (2 pi 0.9 deviation_hz), so the
 *              standard multiplex 0.45 (L + R) + 0.45 (L - R) cos 2 theta + 0.1 cos theta at peak deviation reads 1.0 at full
 *              scale; sigma is the stereo flag of the frame holding n (sigma = 0: L == R exactly).
 *   status     frame f covers n in [f L, (f + 1) L): w = arg sum p[n] conj(p[n - 1]) over the frame's L - 1 adjacent pairs,
 *              C = |mean p[n] exp(-j w (n - f L))|^2, T = mean |p[n]|^2; pilot_hz = w Fc / 2 pi, pilot_dev_hz = 2 sqrt(C)
 *              Fc / 2 pi, pilot_snr_db = 10 log10(C / (T - C)), 100 where T - C <= 0.
 *   flag       turns on when pilot_snr_db >= pilot_on_db, pilot_dev_hz >= pilot_min_hz and |pilot_hz - 19000| <=
 *              pilot_tol_hz all hold; turns off when pilot_snr_db < pilot_off_db or one of the other two fails.  The state
 *              is carried across frames and calls (off when a slot is set); force_mono pins sigma (and status.stereo) to 0.
 * Samples that do not complete a frame are carried to the next call, so the same composite split differently into calls
 * or blocks gives the same bits.
 * Limits (refused by kq_wfm_create with the reason in kq_last_error): Fc >= 128000, Fo >= 32000, Da divides L and M - 1,
 * M odd, N even, 2^a 3^b 5^c 7^d and <= 16384, and 15 kHz + the transition band 2 Fc sqrt(1 + kaiser_beta^2) / M (the
 * window's main lobe) <= 19 kHz - pilot_bw / 2; max_slots <= 4096.
 * Device memory per slot: (Rx + Rd) 4 + Fmax 20 bytes, Rx = max_samples + L - 1 + M - 1 + D, Rd = Fmax L + M - 1,
 * Fmax = ceil(max_samples / L): about (2 max_samples + 2 L + 2.5 M) 4 bytes; plus one h_m (N 8 bytes) per distinct deemph_us.
 * Calls: kq_wfm_create touches no device.  kq_wfm_process with device memory is asynchronous on the handle's stream and
 * reads nothing back; with host memory it is synchronous.  kq_wfm_set, kq_wfm_remove and kq_wfm_reset wait for the stream
 * and take effect at the first sample of the next kq_wfm_process.  One lock per handle. */
typedef struct kq_wfm_bank kq_wfm_bank;
typedef struct kq_wfm_config {
  int device;
  int comp_rate;             /* Fc: composite samples per second */
  unsigned decimate;         /* Da: Fo = Fc / Da */
  unsigned L, M;             /* new samples per frame, filter length (odd) */
  float kaiser_beta;         /* window_filter's beta for both responses (make_kaiser convention) */
  float pilot_bw;            /* Hz: width of h_p's passband around 19 kHz */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  size_t max_samples;        /* largest nblocks * block_len of one kq_wfm_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_wfm_config;
typedef struct kq_wfm_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float deviation_hz;        /* peak deviation of a full-scale multiplex, 75000 for broadcast FM */
  float deemph_us;           /* de-emphasis time constant: 75, 50 or 0 (none) */
  float pilot_on_db, pilot_off_db;  /* hysteresis thresholds on pilot_snr_db, off <= on */
  float pilot_min_hz;        /* least pilot_dev_hz for stereo */
  float pilot_tol_hz;        /* largest |pilot_hz - 19000| for stereo */
  int force_mono;
} kq_wfm_params;
typedef struct kq_wfm_status {
  float pilot_hz, pilot_dev_hz, pilot_snr_db;
  int32_t stereo;            /* sigma of the frame */
} kq_wfm_status;

kq_wfm_bank *kq_wfm_create(const kq_wfm_config *cfg);
int kq_wfm_destroy(kq_wfm_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample (zero history, flag off) */
int kq_wfm_set(kq_wfm_bank *bank, unsigned slot, const kq_wfm_params *params);
/* The slot stops from the next call */
int kq_wfm_remove(kq_wfm_bank *bank, unsigned slot);
/* Composite sample i of block k for row r is comp[r src_stride + k row_stride + i], i < block_len, k < nblocks (a receiver
 * bank's audio plane: row_stride = 2 olen, block_len = olen, src_stride = max_blocks 2 olen).  Returns F, the frames
 * completed in this call (the same for every slot, known without the device).  out[slot out_stride + 2 j + {0, 1}] holds
 * L / R for j < F L / Da; status[slot status_stride + f] for f < F (strides in floats / in kq_wfm_status); either may be
 * NULL.  on_device != 0: comp, out and status are device memory and the call is asynchronous on the handle's stream. */
int kq_wfm_process(kq_wfm_bank *bank, const float *comp, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, float *out, size_t out_stride, kq_wfm_status *status,
                   size_t status_stride);
int kq_wfm_sync(kq_wfm_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings */
int kq_wfm_reset(kq_wfm_bank *bank);

/* --- RDS / RBDS decoder bank -------------------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each reading the 57 kHz data subcarrier of one broadcast FM composite (the input of kq_wfm_*:
 * a flat FM channel's discriminator output in rad/sample at Fc = comp_rate; a receiver bank's audio plane can be decoded
 * in place on its stream after kq_bank_join) and giving RDS groups: four 16-bit blocks each, with a mask of the blocks
 * whose checkword held.  There is no error correction.  The reference has no RDS decoder: the algorithm is defined here.
 * Geometry: Dr = decimate, Fr = Fc / Dr, frames of L new samples, filter length M (odd), N = L + M - 1, Lr = L / Dr,
 * spb = Fr / 1187.5 (samples of z per bit).  Per slot, x[n] is the composite; n counts samples since create or
 * kq_rds_reset on a grid shared by every slot, and x[n] = 0 before the slot was set.
 *   response   h_r: the ideal response R(f) sampled on the N bins and shaped by window_filter's procedure as for kq_wfm_*
 *              (filter.c:365-413, in double, make_kaiser(M, kaiser_beta), used as float).  With g = f - 57000 and
 *              t_d = 1 / 1187.5: R = -j sin(pi g t_d / 2) cos(pi g t_d / 4) for |g| <= 2 / t_d = 2375 Hz, 0 elsewhere: the
 *              matched filter of the shaped biphase symbol of IEC 62106; one-sided, so the taps are complex.
 *   baseband   z[k] = (h_r * x)[k Dr] exp(-j 2 pi ((57000 k Dr) mod Fc) / Fc), k on the global grid; frame f owns
 *              k in [f Lr, (f + 1) Lr).
 *   sums       over the frame's Lr samples: S_f = sum z[k]^2, E_f = sum |z[k]|^2 exp(-j 2 pi ((2375 k) mod 2 Fr) / 2 Fr),
 *              P_f = sum |z[k]|^2.
 *   tracker    sequential over frames, state zero when a slot is set.  alpha = 1 - exp(-L / (Fc track_ms 1e-3));
 *              A_f = A_{f-1} + alpha (S_f - A_{f-1}), B_f likewise from E_f.  Carrier: w = arg A_f - 2 phi_{f-1},
 *              phi_f = phi_{f-1} + (w - 2 pi rint(w / 2 pi)) / 2, wrapped into (-pi, pi].  Bit clock:
 *              u = -arg(B_f) / 2 pi - tau_{f-1}, tau_f = tau_{f-1} + u - rint(u): unwrapped, never reduced.
 *   bits       bit i is sampled at t_i = (i + tau_f) spb, in samples of z.  In frame f, from the next unsampled i, bits are
 *              taken while t_i + 1 < (f + 1) Lr; consecutive i are neither skipped nor repeated.  The first i of a slot is
 *              the least with t_i >= f_s Lr, f_s the slot's first frame.  With k0 = floor(t_i), r = t_i - k0:
 *              y_i = Re((z[k0] + r (z[k0 + 1] - z[k0])) exp(-j phi_f)), c_i = (y_i < 0), data bit b_i = c_i xor c_{i-1}
 *              (c before the first: 0).
 *   blocks     crc10(w) = remainder of w x^10 modulo x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 (0x5B9), w of 16 bits.  A 26-bit
 *              word is (info << 10) | (crc10(info) xor offset); offsets A 0x0FC, B 0x198, C 0x168, C' 0x350, D 0x1B4 at
 *              positions 0, 1, 2, 2, 3.  Per bit reg = (reg << 1 | b) mod 2^26; once 26 bits are in,
 *              s = crc10(reg >> 10) xor (reg & 0x3FF), and a "hit" is an offset equal to s.
 *   unsynced   every hit is remembered (bit count, offset, info word).  Sync is taken when a hit comes exactly 26 bits
 *              after the remembered one at the remembered position + 1 mod 4: a fresh group record opens, the remembered
 *              word goes into its place with its ok bit if the new position is above 0, the new word goes in with its ok
 *              bit, C' sets version_b, and position 3 emits the group.
 *   synced     every 26 bits the word is stored at the expected position whether good or not; it is good if the hit's
 *              position is the expected one: that sets its ok bit and zeroes `bad`, anything else increments `bad`.
 *              Position 3 emits the group and opens a new record.  bad >= lose_after drops sync, the remembered hit and
 *              the open record.  blocks_ok / blocks_bad count the words stored with / without their ok bit since the set.
 * Samples that do not complete a frame are carried to the next call, so the same composite split differently into calls
 * or blocks gives the same bits.
 * Limits (refused by kq_rds_create with the reason in kq_last_error): Fc >= 128000; Dr divides Fc, L and M - 1; Fr >= 9500;
 * M odd; N even, 2^a 3^b 5^c 7^d and <= 16384; (57000 N) mod Fc = 0 (the subcarrier sits on a bin, so the mix is a bin shift
 * and a per-frame phase from integer arithmetic); (M - 1) / Fc >= 3 / 1187.5; 59375 Hz + the transition band
 * 2 Fc sqrt(1 + kaiser_beta^2) / M <= Fc / 2; max_slots <= 4096.  kq_rds_set refuses track_ms <= 0 and lose_after < 1.
 * Device memory per slot: Rx 4 + Rz 8 + Fmax 40 bytes, Rx = max_samples + L - 1 + M - 1, Rz = Fmax Lr + ceil(spb) + 2,
 * Fmax = ceil(max_samples / L).
 * Calls: kq_rds_create touches no device.  kq_rds_process with device memory is asynchronous on the handle's stream and
 * reads nothing back; with host memory it is synchronous.  kq_rds_set, kq_rds_remove and kq_rds_reset wait for the stream
 * and take effect at the first sample of the next kq_rds_process.  One lock per handle. */
typedef struct kq_rds_bank kq_rds_bank;
typedef struct kq_rds_config {
  int device;
  int comp_rate;             /* Fc: composite samples per second */
  unsigned decimate;         /* Dr: Fr = Fc / Dr */
  unsigned L, M;             /* new samples per frame, filter length (odd) */
  float kaiser_beta;         /* window_filter's beta (make_kaiser convention) */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  size_t max_samples;        /* largest nblocks * block_len of one kq_rds_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_rds_config;
typedef struct kq_rds_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float track_ms;            /* time constant of the carrier and bit-clock tracker, 20 by default */
  int lose_after;            /* consecutive bad blocks that drop sync, 10 by default */
} kq_rds_params;
typedef struct kq_rds_group {
  uint16_t block[4];
  uint8_t ok;                /* bit p: the block at position p passed its check */
  uint8_t version_b;         /* the block at position 2 came with offset C' */
  uint16_t reserved;
  uint32_t bit;              /* bits decoded since the slot was set, at the group's last bit */
} kq_rds_group;
typedef struct kq_rds_status {
  float phase, timing;       /* phi_f (rad), tau_f (bits) */
  float level;               /* sqrt(P_f / Lr) */
  int32_t synced;
  uint32_t blocks_ok, blocks_bad;
} kq_rds_status;

kq_rds_bank *kq_rds_create(const kq_rds_config *cfg);
int kq_rds_destroy(kq_rds_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample */
int kq_rds_set(kq_rds_bank *bank, unsigned slot, const kq_rds_params *params);
/* The slot stops from the next call */
int kq_rds_remove(kq_rds_bank *bank, unsigned slot);
/* The bound on groups per slot of a call of nsamples (0 and an error for no bank): ceil(nsamples 1187.5 / Fc) / 104 + 2, or
 * more where a call can emit more.  A call completes F <= (nsamples + L - 1) / L frames, up to L - 1 of whose samples were
 * carried in, and tau moves by at most half a bit per frame, so it decodes fewer than (nsamples + L - 1) 1187.5 / Fc + F / 2
 * + 1 bits and emits at most floor(that / 104) + 1 groups: the bound is the larger of the two, and no group is ever dropped. */
size_t kq_rds_max_groups(const kq_rds_bank *bank, size_t nsamples);
/* Composite addressed as in kq_wfm_process.  Returns F, the frames completed in this call.  groups[slot groups_stride + g]
 * holds group g for g < counts[slot] and zeros from there to kq_rds_max_groups(bank, nblocks block_len), below which
 * groups_stride is refused; status[slot status_stride + f] for f < F (strides in records).  Any output may be NULL; nothing is written for an empty slot.
 * on_device != 0: every pointer is device memory and the call is asynchronous on the handle's stream. */
int kq_rds_process(kq_rds_bank *bank, const float *comp, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_rds_group *groups, size_t groups_stride, uint32_t *counts,
                   kq_rds_status *status, size_t status_stride);
/* The last call's z of a slot (F Lr complex samples, cap_complex at most) to host memory; synchronous; returns the count */
int kq_rds_pull_baseband(kq_rds_bank *bank, unsigned slot, float *dst_re_im, size_t cap_complex);
int kq_rds_sync(kq_rds_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings */
int kq_rds_reset(kq_rds_bank *bank);

/* --- monitor mixer bank ------------------------------------------------------------------------------------------------
 * Up to 65536 sessions, each one row of PCM (mono or stereo) with a gain, a stereo position and a mute switch
 * (monitor.c:433-450), summed into up to 256 stereo buses (monitor.c:475-496 has one).  A receiver bank's audio plane
 * (kq_bank_audio_device_ptr) is mixed in place on its stream after kq_bank_join(bank); kq_wfm_*'s output likewise.
 * n counts frames since create or kq_mon_reset, on one grid for all sessions.  Per session, in float:
 *   gains      gl = gain (1 - pan) / 2, gr = gain (1 + pan) / 2                                      (monitor.c:440-441)
 *   delays     dl = pan > 0 ? round(pan 0.001 samprate) : 0, dr = pan < 0 ? round(-pan 0.001 samprate) : 0, in double with
 *              C's round (monitor.c:444-447): the less favoured side comes up to 1 ms late
 *   samples    xl[n], xr[n]: equal for a mono session, zero before the session was set.  KQ_MON_S16BE words w are
 *              SCALE * (short)ntohs(w) as a float product, SCALE = 1.f / SHRT_MAX                    (monitor.c:88,492)
 * The members of bus b are its unmuted sessions in ascending slot order, m_0 .. m_{K-1}.  (monitor.c adds a muted stream
 * with gain 0; here it is left out, so a NaN from a channel nobody listens to never reaches the bus.)  Chunk c holds
 * members 64 c .. 64 c + 63; its partial is P_c = the fold acc = fmaf(gl_m, xl_m[n - dl_m], acc) from 0.0f in member order,
 * and the bus sample is 0.0f + P_0 + P_1 + ... in chunk order, by float additions; the right side likewise with gr, xr, dr.
 * This order is part of the contract: it makes the bits independent of how the stream is cut into calls and blocks and
 * of every session in another bus.  An empty bus gives zeros.
 * H = round(0.001 samprate) frames of every session's input (muted ones too) are carried across calls, so a call may bring
 * fewer than H frames, or one.
 * pcm is out through scaleclip (audio.c:22-28: >= 1 gives SHRT_MAX, <= -1 SHRT_MIN, else truncation of SHRT_MAX x; NaN
 * gives 0) in network byte order.  status, one record per bus and call: peak_* the largest |sample| of the call, clipped
 * the number of int16 words equal to SHRT_MAX or SHRT_MIN, sessions = K, active the members with any non-zero input
 * sample in this call (those audio.c:101-104 would not have suppressed).
 * Limits (refused with -1 / NULL and the reason in kq_last_error, before any device call): samprate 8000 .. 384000,
 * max_sessions 1 .. 65536, max_buses 1 .. 256, max_samples >= 1; slot < max_sessions, bus < max_buses, channels 1 or 2,
 * gain finite and >= 0, |pan| <= 1; kq_mon_adjust / kq_mon_remove of an empty slot; nblocks block_len > max_samples;
 * nblocks > 1 with a block (2 block_len elements where a stereo session is set) longer than row_stride; an unknown format.
 * Device memory: max_sessions (8 H + 68) bytes of history and tables, and (max_sessions / 64 + max_buses) 8208 bytes of
 * chunk partials (1024 frames at a time, whatever max_samples is); host-memory calls add their staging buffers.
 * Calls: kq_mon_create, kq_mon_set, kq_mon_adjust and kq_mon_remove touch no device; they and kq_mon_reset take effect at
 * the first frame of the next kq_mon_process, which uploads the tables when they changed.  kq_mon_process with device
 * memory is asynchronous on the handle's stream and reads nothing back; with host memory it is synchronous.  One lock per
 * handle. */
enum kq_mon_format { KQ_MON_F32 = 0, KQ_MON_S16BE = 1 };  /* float, or int16 in network byte order (audio.c's PCM) */
typedef struct kq_mon_bank kq_mon_bank;
typedef struct kq_mon_config {
  int device;
  int samprate;              /* frames per second of every input and of the buses */
  unsigned max_sessions;     /* slots 0 .. max_sessions - 1 (limit 65536) */
  unsigned max_buses;        /* buses 0 .. max_buses - 1 (limit 256) */
  size_t max_samples;        /* largest nblocks * block_len of one kq_mon_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_mon_config;
typedef struct kq_mon_params {
  unsigned source;           /* input row this session plays (a receiver bank's channel index) */
  unsigned bus;
  int channels;              /* 1: mono, 2: interleaved L, R */
  float gain;                /* linear, >= 0 */
  float pan;                 /* -1 (left) .. +1 (right) */
  int muted;
} kq_mon_params;
typedef struct kq_mon_status {
  float peak_left, peak_right;
  int32_t clipped, sessions, active;
} kq_mon_status;

kq_mon_bank *kq_mon_create(const kq_mon_config *cfg);
int kq_mon_destroy(kq_mon_bank *bank);
/* Put a session in `slot` (or replace the one there): a cold start, zero history */
int kq_mon_set(kq_mon_bank *bank, unsigned slot, const kq_mon_params *params);
/* monitor.c's keys: new gain, position and mute switch of the session in `slot`; its history is kept */
int kq_mon_adjust(kq_mon_bank *bank, unsigned slot, float gain, float pan, int muted);
int kq_mon_remove(kq_mon_bank *bank, unsigned slot);
/* T = nblocks block_len frames per session.  Block k of row r starts at audio[r src_stride + k row_stride]: a mono session
 * reads block_len values there, a stereo one 2 block_len interleaved L, R (a receiver bank's plane: src_stride =
 * max_blocks 2 olen, row_stride = 2 olen, block_len = olen; kq_wfm_*'s output is one block of pairs); strides in elements
 * of `format`.  Returns T.  out[b out_stride + 2 j + {0, 1}] is bus b's L / R for j < T (stride in floats), pcm[b
 * pcm_stride + 2 j + {0, 1}] the same as int16 in network byte order, status[b] one record per bus; all max_buses buses are
 * written, and any of the three may be NULL.  on_device != 0: every pointer is device memory and the call is asynchronous
 * on the handle's stream. */
int kq_mon_process(kq_mon_bank *bank, const void *audio, int format, size_t src_stride, size_t row_stride,
                   unsigned block_len, unsigned nblocks, int on_device, float *out, size_t out_stride, int16_t *pcm,
                   size_t pcm_stride, kq_mon_status *status);
int kq_mon_sync(kq_mon_bank *bank);
/* Frame index back to 0; every session restarts with zero history and its settings */
int kq_mon_reset(kq_mon_bank *bank);

/* --- baseband FSK / GMSK packet decoder bank ------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each reading HDLC frames from the discriminator output of one flat FM channel (rad/sample at
 * Fs = samprate; a receiver bank's audio plane can be decoded in place on its stream after kq_bank_join): 9600 bit/s G3RUH
 * packet (scrambled, NRZI, AX.25) and AIS (GMSK 9600 bit/s, NRZI, unscrambled, the same framing and 16-bit FCS), or any
 * other rate with 4 baud <= Fs <= 40 baud.  The reference has no such decoder (packet.c is AFSK-1200): the algorithm is
 * defined here.  Everything after the quantiser is integer arithmetic, so the bits do not depend on how sums are ordered.
 * Per slot, x[n] is its input row; n counts samples since create or kq_fsk_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  K = taps, W = rint(window_bits Fs / baud).
 *   quantise   q[n] = clamp(rint(x[n] input_scale), -32767, 32767): one float multiply, round to nearest even; NaN reads
 *              as 0.  input_scale 4096 suits rad/sample.  A KQ_PCM_S16BE word w (network byte order, two's complement) is
 *              taken as q itself, -32768 as -32767.
 *   low-pass   h[k] = sinc(2 cutoff_hz / Fs (k - (K - 1) / 2)) w[k], w = make_kaiser(K, kaiser_beta) (filter.c:337-357), in
 *              double, scaled to sum h = 1; hq[k] = rint(32768 h[k]) as int16 (kq_fsk_get_taps); y[n] = sum_k hq[k] q[n - k] in
 *              int32.  A design with sum |hq| > 65535 is refused, so y cannot overflow.
 *   threshold  c2[n] = max(y[n - W + 1 .. n]) + min(y[n - W + 1 .. n]), d[n] = (2 y[n] > c2[n]) in 64 bits: the mid level of
 *              the last window_bits bits takes out DC and tuning offset.  d = 0 before the stream starts.
 *   bit clock  s: int32, 0 when the slot is set; inc = rint(2^32 baud / Fs).  Per sample n in order: if d[n] != d[n - 1],
 *              s = s - (s >> pll_shift) (arithmetic shift); then t = s + inc; if t >= 2^31, s = t - 2^32 and a channel bit
 *              c = d[n] is taken, else s = t.
 *   bits       scrambled slots (G3RUH, 1 + x^12 + x^17, self-synchronising): u = c xor sr<16> xor sr<11>, then
 *              sr = (sr << 1 | c) & 0x1FFFF; else u = c.  Data bit b = (u == u_prev) (NRZI).  sr = 0, u_prev = 0 at the set.
 *   HDLC       state ones, in_frame, nbits (saturating at 2^31 - 1) and the open frame of max_frame_bytes bytes, filled LSB
 *              first; bits beyond it are counted in nbits and not stored.
 *              b = 1: ones = min(ones + 1, 7); at 7, aborts += in_frame and in_frame = 0; below 7, in a frame, a 1 is appended.
 *              b = 0: ones == 6 is a flag: if in_frame, nb = nbits - 7 is a candidate when nb >= 8 min_bytes; it is good when
 *              nb mod 8 == 0, nb / 8 <= max_frame_bytes and the CRC-16/X.25 of its nb / 8 bytes leaves 0xf0b8 (ax25.c:138-156
 *              crc_good): frames_good += 1 and the frame goes to the slot's arena, or dropped += 1 when that holds
 *              max_frames; any other candidate: frames_bad += 1.  Then in_frame = 1, nbits = 0.  ones == 5: a stuffed
 *              zero, dropped.  ones < 5, in a frame: a 0 is appended.  Always ones = 0.
 *   record     the bytes (body + FCS, as kq_afsk_pull_frame gives them), length, end_sample (n of the sample at which the
 *              closing flag's last bit was taken: AIS slot timing) and end_bit (bits taken since the set, that one included).
 * Every sample of a call is consumed in that call; carried are the last K - 1 + W - 1 + 63 values of q, s, sr, u_prev, d
 * of the last sample, the deframer and the open frame, so the same stream split differently into calls or blocks gives the
 * same bits, records and status.  d is packed 64 samples to a word on the grid (bit n mod 64 of word n / 64); a call that
 * starts inside a word computes that word again from the carried q.
 * Limits (refused by kq_fsk_create / kq_fsk_set with the reason in kq_last_error, before any HIP call): 4 baud <= Fs <=
 * 40 baud (the algorithm decodes cleanly at 4.07 samples per bit and fails at 2.5); K odd, 3..127; 2 <= W <= 1024;
 * 0 < cutoff_hz < Fs / 2; kaiser_beta finite and >= 0; 1 <= pll_shift <= 8; input_scale > 0; max_slots 1..4096; max_frames
 * 1..4096; 8 <= max_frame_bytes <= 1024; max_samples 1..2^28; 4 <= min_bytes <= max_frame_bytes.
 * Device memory per slot: 4 (K + W + 61) bytes of q (two copies), 8 (max_samples / 64 + 2) of d, max_frame_bytes of open
 * frame, max_frames (max_frame_bytes + 16) of arena and 96 of state and tables.
 * Calls: kq_fsk_create touches no device.  kq_fsk_process with device memory is asynchronous on the handle's stream and
 * reads nothing back; with host memory it is synchronous.  kq_fsk_set, kq_fsk_remove and kq_fsk_reset wait for the stream
 * and take effect at the first sample of the next kq_fsk_process.  One lock per handle. */
typedef struct kq_fsk_bank kq_fsk_bank;
typedef struct kq_fsk_config {
  int device;
  int samprate;              /* Fs: input samples per second */
  int baud;
  unsigned taps;             /* K: low-pass length (odd) */
  float cutoff_hz;           /* 0.6 baud is a good choice */
  float kaiser_beta;         /* make_kaiser convention */
  float window_bits;         /* threshold window, in bits: W = rint(window_bits Fs / baud) */
  float input_scale;
  int pll_shift;
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  unsigned max_frames;       /* arena places per slot between kq_fsk_clear_frames calls */
  unsigned max_frame_bytes;  /* longest frame, FCS included */
  size_t max_samples;        /* largest nblocks * block_len of one kq_fsk_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_fsk_config;
typedef struct kq_fsk_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  int scrambled;             /* 1: G3RUH, 0: plain NRZI (AIS) */
  unsigned min_bytes;        /* shortest candidate, FCS included; 8 by default */
} kq_fsk_params;
typedef struct kq_fsk_status {   /* counters since the slot was set */
  uint32_t bits;
  uint32_t frames_good, frames_bad, aborts, dropped;
  int32_t pll_phase;         /* s */
  int32_t in_frame;
  uint32_t level;            /* max - min of y over the window at the call's last sample */
} kq_fsk_status;
typedef struct kq_fsk_frame_info {
  uint32_t length;
  uint32_t end_bit;
  uint64_t end_sample;
} kq_fsk_frame_info;

kq_fsk_bank *kq_fsk_create(const kq_fsk_config *cfg);
int kq_fsk_destroy(kq_fsk_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty */
int kq_fsk_set(kq_fsk_bank *bank, unsigned slot, const kq_fsk_params *params);
/* The slot stops from the next call; its arena stays readable */
int kq_fsk_remove(kq_fsk_bank *bank, unsigned slot);
/* Input addressed as in kq_wfm_process, in elements of `format` (KQ_PCM_F32 or KQ_PCM_S16BE).  status[slot status_stride]
 * is the slot's record after the call's last sample (stride in records, may be NULL; nothing is written for an empty
 * slot).  Returns 0.  on_device != 0: src and status are device memory and the call is asynchronous on the handle's
 * stream. */
int kq_fsk_process(kq_fsk_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_fsk_status *status, size_t status_stride);
/* Frames in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_fsk_pull_counts(kq_fsk_bank *bank, uint32_t *counts);
/* Copies frame `index` of `slot` (at most cap bytes) and its record (info may be NULL); returns its length, or -1 */
int kq_fsk_pull_frame(kq_fsk_bank *bank, unsigned slot, unsigned index, unsigned char *dst, size_t cap,
                      kq_fsk_frame_info *info);
/* Empties every arena (on the handle's stream); the status counters go on */
int kq_fsk_clear_frames(kq_fsk_bank *bank);
/* hq (at most cap words); returns K */
int kq_fsk_get_taps(const kq_fsk_bank *bank, int16_t *dst, size_t cap);
int kq_fsk_sync(kq_fsk_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings */
int kq_fsk_reset(kq_fsk_bank *bank);

/* --- POCSAG pager decoder bank -------------------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each reading POCSAG pages (direct FSK at 512, 1200 or 2400 bit/s on 12.5 / 25 kHz channels;
 * the amateur DAPNET transmitters use it too) from the discriminator output of one flat FM channel, as kq_fsk_* reads
 * packet: a receiver bank's audio plane can be decoded in place on its stream after kq_bank_join.  The bit rate is per
 * bank, as in kq_fsk_*: a channel that carries 512, 1200 and 2400 bit/s traffic is read by three banks on the same plane
 * and stream.  The reference has no such decoder: the algorithm is defined here.  All integer after the quantiser.
 * Front end: quantise, low-pass, threshold and bit clock exactly as kq_fsk_* defines them above (the same code), with
 * K = taps, W = rint(window_bits Fs / baud), Fs = samprate (a double, so that 39 062.5 is exact).  There is no
 * descrambler and no NRZI: the channel bit c that the bit clock takes goes to the deframer as it is.
 *   constants  FSC = 0x7CD215D8 (frame sync), IDLE = 0x7A89C197, generator g(x) = x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
 *              (0x769).  A codeword is 32 bits, sent MSB first: bit 31 flag, bits 30..11 payload, bits 10..1 the BCH check
 *              over bits 31..11 (bits 31..1 as a polynomial are a multiple of g), bit 0 even parity over the whole word.
 *              FSC and IDLE are codewords.
 *   correct    For a 32-bit word x: syn = bits 31..1 of x as a polynomial modulo g (10 bits), par = popcount(x) & 1.  A
 *              table of 2048 words maps (syn << 1 | par) to the error pattern of weight <= 2 over the 32 bits that gives
 *              that pair (1 + 32 + 496 patterns, distinct because the extended code has minimum distance 6), every other
 *              entry to "uncorrectable".  (v, e) = (x xor pattern, its weight); kq_pag_correct is this on the host, from
 *              the table the device gets.  Every word with three flipped bits is uncorrectable.
 *   state      sh (32 bits), synced, inv, cnt, pos, miss and the open page; all zero at the set.
 *   hunting    (synced == 0) per channel bit c: sh = (sh << 1) | c.  If popcount(sh ^ FSC) <= 2: synced = 1, inv = 0; else
 *              if popcount(~sh ^ FSC) <= 2: synced = 1, inv = 1.  On either: cnt = pos = miss = 0, syncs += 1, batches += 1.
 *   synced     sh shifts as above and cnt += 1; at cnt == 32 the word x = inv ? ~sh : sh is taken and cnt = 0.
 *   sync word  (pos == 16) popcount(x ^ FSC) <= 2: batches += 1, miss = 0.  Else sync_missed += 1, miss += 1, and at
 *              miss == 2 sync is dropped: synced = 0 (inv stays as it is until the next sync), and an open page closes
 *              with flag LOST.  Then pos = 0.
 *   codeword   (pos 0..15) x is corrected to (v, e), then pos += 1 (pos_before is pos ahead of that).
 *              Uncorrectable: words_bad += 1; if a page is open and holds fewer than max_page_words words, bits 30..11 of
 *              x are appended with error code 3 and the page gets flag BAD; else nothing more.
 *              Otherwise words_good += 1 (e == 0) or words_fixed += 1 (e = 1, 2), and
 *                v == IDLE: an open page closes.
 *                bit 31 of v clear (address): an open page closes; then one opens with ric = ((v >> 13) & 0x3FFFF) << 3 |
 *                  (pos_before >> 1), function = (v >> 11) & 3, nwords = 0, flags = 0, errors = e.
 *                bit 31 set (message): with no open page, orphans += 1.  Else, if the page holds fewer than
 *                  max_page_words, bits 30..11 of v are appended with error code e and errors += e; if it is full it
 *                  closes with flag FULL at this word, and the word counts in orphans.
 *   record     each message word as 3 bytes, big-endian: bits 19..0 the payload, bits 21..20 the error code (0, 1, 2, or
 *              3 for uncorrectable); ric, function, nwords, flags (LOST = 1, FULL = 2, BAD = 4), errors (the sum of e
 *              over the address and the corrected message words) and end_sample (n of the sample at which the last bit
 *              of the page's last stored codeword -- the address, or the last word appended -- was taken).
 *   closing    pages += 1 and the page goes to the slot's arena, or dropped += 1 when that holds max_pages.  A page open
 *              at the end of a call is carried.
 * Every sample of a call is consumed in that call, and what is carried is the front end's, the state above and the open
 * page, so the same stream split differently into calls or blocks -- calls that start inside a 64-sample word, that end
 * inside a codeword, a batch or a page -- gives the same records and status.
 * Run lengths: the threshold is the mid level of the last window_bits bits, so a run of equal bits longer than the window
 * loses it.  Traffic keeps its runs short (21 bits at most in the trains this was tried on, against windows of 20 to 24
 * bits); the 96 ones of three message words 0xFFFFF in a row cannot be decoded at any window the limits allow.  W <= 1024
 * leaves at most 25 bits of window at 40 samples per bit: 20 samples per bit or fewer are recommended, and 512 bit/s from a
 * 48 kHz plane goes through kq_rsmp_*.  cutoff_hz 0.75 baud, pll_shift 3 and window_bits min(24, 1024 baud / Fs - 0.5)
 * are good choices.
 * Limits (refused by kq_pag_create / kq_pag_set with the reason in kq_last_error, before any HIP call): those of
 * kq_fsk_* (4 baud <= Fs <= 40 baud; K odd, 3..127; 2 <= W <= 1024; 0 < cutoff_hz < Fs / 2; kaiser_beta finite and >= 0;
 * 1 <= pll_shift <= 8; input_scale > 0; max_slots 1..4096; max_samples 1..2^28; sum |hq| <= 65535), max_pages 1..4096,
 * max_page_words 1..256.
 * Device memory per slot: 4 (K + W + 61) bytes of q (two copies), 8 (max_samples / 64 + 2) of d, 3 max_page_words of open
 * page, max_pages (3 max_page_words + 32) of arena and 128 of state and tables; 8 KiB of correction table per bank.
 * Calls: as kq_fsk_*.  kq_pag_create touches no device; kq_pag_correct never does. */
#define KQ_PAG_FSC 0x7CD215D8u
#define KQ_PAG_IDLE 0x7A89C197u
#define KQ_PAG_LOST 1u
#define KQ_PAG_FULL 2u
#define KQ_PAG_BAD 4u
typedef struct kq_pag_bank kq_pag_bank;
typedef struct kq_pag_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  int baud;                  /* 512, 1200 or 2400 */
  unsigned taps;             /* K: low-pass length (odd) */
  float cutoff_hz;           /* 0.75 baud is a good choice */
  float kaiser_beta;         /* make_kaiser convention */
  float window_bits;         /* threshold window, in bits: W = rint(window_bits Fs / baud) */
  float input_scale;
  int pll_shift;
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  unsigned max_pages;        /* arena places per slot between kq_pag_clear_pages calls */
  unsigned max_page_words;   /* message words a page can hold */
  size_t max_samples;        /* largest nblocks * block_len of one kq_pag_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_pag_config;
typedef struct kq_pag_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
} kq_pag_params;
typedef struct kq_pag_status {   /* counters since the slot was set */
  uint32_t bits;
  uint32_t syncs;            /* times sync was found while hunting */
  uint32_t batches;          /* sync words accepted, those included */
  uint32_t sync_missed;
  uint32_t words_good, words_fixed, words_bad;
  uint32_t orphans, pages, dropped;
  int32_t pll_phase;         /* s */
  int32_t synced;
  int32_t inverted;          /* inv */
  uint32_t level;            /* max - min of y over the window at the call's last sample */
} kq_pag_status;
typedef struct kq_pag_page_info {
  uint32_t ric;
  uint32_t function;
  uint32_t nwords;
  uint32_t flags;
  uint32_t errors;
  uint32_t reserved;         /* 0 */
  uint64_t end_sample;
} kq_pag_page_info;

kq_pag_bank *kq_pag_create(const kq_pag_config *cfg);
int kq_pag_destroy(kq_pag_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty */
int kq_pag_set(kq_pag_bank *bank, unsigned slot, const kq_pag_params *params);
/* The slot stops from the next call; its arena stays readable */
int kq_pag_remove(kq_pag_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_fsk_process */
int kq_pag_process(kq_pag_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_pag_status *status, size_t status_stride);
/* Pages in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_pag_pull_counts(kq_pag_bank *bank, uint32_t *counts);
/* Copies the words of page `index` of `slot` (3 bytes each, at most cap bytes) and its record (info may be NULL); returns
 * 3 nwords, or -1 */
int kq_pag_pull_page(kq_pag_bank *bank, unsigned slot, unsigned index, unsigned char *dst, size_t cap,
                     kq_pag_page_info *info);
/* Empties every arena (on the handle's stream); the status counters go on */
int kq_pag_clear_pages(kq_pag_bank *bank);
/* hq (at most cap words); returns K */
int kq_pag_get_taps(const kq_pag_bank *bank, int16_t *dst, size_t cap);
int kq_pag_sync(kq_pag_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings */
int kq_pag_reset(kq_pag_bank *bank);
/* Host only: the correction of one received word by the table the device gets.  Returns the number of bits changed (0, 1
 * or 2) with the codeword in *fixed (may be NULL), or -1 (uncorrectable; *fixed is left alone) */
int kq_pag_correct(uint32_t word, uint32_t *fixed);

/* --- tone signalling decoder bank -----------------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each reading the in-band tone signalling of one voice channel from its audio row (a receiver
 * bank's audio plane can be decoded in place on its stream after kq_bank_join): DTMF, the sequential five-tone selective
 * calls (ZVEI, CCIR, EIA ...), two-tone sequential paging.  One bank decodes one tone plan: a channel that carries DTMF
 * and ZVEI is read by two banks on the same plane and stream, as kq_fsk_* and kq_pag_* read several bit rates.  The
 * reference has no such decoder: the algorithm is defined here.  Everything after the quantiser is exact integer
 * arithmetic, so no result depends on how sums are ordered or how the stream is cut into calls.
 * Per slot, x[n] is its input row; n counts samples since create or kq_tone_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len, T = ntones; block k is the samples [k B, (k + 1) B).
 *   quantise   as kq_fsk_*: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to nearest even,
 *              NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.
 *   table      C[j] = rint(32767 cos(2 pi j / 1024)) as int16, j = 0..1023, made once on the host in double
 *              (kq_tone_get_table).
 *   correlate  tone t: inc_t = rint(f_t 2^32 / Fs) in double, f_t the float of the config (kq_tone_get_incs);
 *              ph_t(n) = (n inc_t) mod 2^32 -- no oscillator state is carried -- and j = ph_t(n) >> 22.  Per block
 *              I_t = sum q[n] C[j], Q_t = sum q[n] C[(j - 256) & 1023], E = sum q[n]^2: exact integers in 64 bits.
 *              a = I_t >> 15, b = Q_t >> 15 (arithmetic shifts), P_t = a^2 + b^2 as uint64.  With B <= 4096: |I| < 2^42,
 *              P < 2^55, R = E B < 2^54.
 *   decide     at every completed block.  The tones are one or two groups of consecutive entries: the first group0, then
 *              group1 (DTMF: low and high; selective calling: one group).  Per group: best = the lowest index that attains
 *              the largest P, P2 = the largest P of the group's other tones, 0 if it has no other.  The block is valid
 *              iff E >= min_ms B; in every group P_best >= (R >> 8) frac and P_best >= (P2 >> 4) ratio; and with two groups
 *              max(P_best0, P_best1) <= (min(P_best0, P_best1) >> 4) twist.  Every compare in uint64.  frac is in 1/256 of
 *              R: a pure tone gives about 128, each tone of an equal pair about 64; ratio and twist are in sixteenths.
 *              Symbol s = i0 | i1 << 8, i the best tone's index within its group, i1 = 0 with one group; an invalid block
 *              gives s = -1.
 *   runs       per slot cur (-1 at the set), run, start, peak.  Per block with symbol s: if s == cur, run += 1 (saturating
 *              at 2^32 - 1) and peak = max(peak, E).  Otherwise the old run closes: if cur >= 0 and run >= min_blocks,
 *              events += 1 and the run goes to the slot's arena as an event, or dropped += 1 when that holds max_events;
 *              then cur = s, run = 1, start = k, peak = E.
 *   event      symbol, blocks = run, start_sample = start B, peak.
 * An open run is no event until it ends; the status shows cur and run, so a client sees a long tone while it lasts.
 * kq_tone_remove and kq_tone_reset discard the open run.  Carried between calls: the I, Q and E of the open block, the
 * run, the counters and the last completed block's P and E; so the same stream split differently into calls or blocks
 * gives the same events, status and powers.
 * Limits (refused by kq_tone_create / kq_tone_set with the reason in kq_last_error, before any HIP call): samprate
 * positive and finite; 8 <= B <= 4096; 1..32 tones in group0 >= 1 and group1 >= 0 with group0 + group1 = ntones;
 * 0 < f_t < Fs / 2; frac 1..128; ratio and twist 16..4095; min_blocks 1..65535; input_scale > 0; max_slots 1..4096;
 * max_events 1..4096; max_samples 1..2^28.
 * Device memory per slot: 24 max_events of arena, 24 (T + 1) + 64 of accumulators, powers and state; 2 KiB of table per
 * bank.
 * Talk-off (speech taken for tones) has not been measured.
 * Calls: as kq_fsk_*.  kq_tone_create touches no device. */
typedef struct kq_tone_bank kq_tone_bank;
typedef struct kq_tone_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per decision block */
  unsigned ntones;           /* T */
  const float *freqs;        /* [T], Hz: the first group's tones, then the second's; copied by kq_tone_create */
  unsigned group0, group1;   /* tones in the first and second group; group1 = 0: one group */
  unsigned min_ms;           /* least mean square of q over a valid block */
  unsigned frac;             /* least P_best, in 1/256 of E B */
  unsigned ratio;            /* least P_best / P2, in sixteenths */
  unsigned twist;            /* largest ratio of the two groups' P_best, in sixteenths */
  unsigned min_blocks;       /* shortest run that makes an event */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  unsigned max_events;       /* arena places per slot between kq_tone_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_tone_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_tone_config;
typedef struct kq_tone_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
} kq_tone_params;
typedef struct kq_tone_status {  /* counters since the slot was set */
  uint32_t blocks;           /* completed */
  uint32_t valid_blocks;
  uint32_t events;           /* runs of min_blocks or more that ended, those dropped included */
  uint32_t dropped;
  int32_t cur;               /* the open run's symbol, -1: none */
  uint32_t run;              /* its blocks so far */
  uint64_t energy;           /* E of the last completed block */
} kq_tone_status;
typedef struct kq_tone_event {
  int32_t symbol;
  uint32_t blocks;
  uint64_t start_sample;
  uint64_t peak;             /* the largest E of the run's blocks */
} kq_tone_event;

kq_tone_bank *kq_tone_create(const kq_tone_config *cfg);
int kq_tone_destroy(kq_tone_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty */
int kq_tone_set(kq_tone_bank *bank, unsigned slot, const kq_tone_params *params);
/* The slot stops from the next call; its arena stays readable */
int kq_tone_remove(kq_tone_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_fsk_process.  powers[slot powers_stride + t] is P_t of the slot's last completed
 * block for t < T, and at t = T its E (stride in values, >= T + 1; may be NULL; nothing is written for an empty slot; all
 * zero until a block has completed).  on_device != 0: powers too is device memory. */
int kq_tone_process(kq_tone_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_tone_status *status, size_t status_stride, uint64_t *powers,
                    size_t powers_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_tone_pull_counts(kq_tone_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_tone_pull_event(kq_tone_bank *bank, unsigned slot, unsigned index, kq_tone_event *event);
/* Empties every arena (on the handle's stream); the status counters and the open runs go on */
int kq_tone_clear_events(kq_tone_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_tone_get_table(const kq_tone_bank *bank, int16_t *dst, size_t cap);
/* inc_t (at most cap words); returns T */
int kq_tone_get_incs(const kq_tone_bank *bank, uint32_t *dst, size_t cap);
int kq_tone_sync(kq_tone_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings */
int kq_tone_reset(kq_tone_bank *bank);

/* --- CW (Morse) decoder bank ------------------------------------------------------------------------------------------------
 * Up to 16384 decoder slots (the slot scaffold takes that number unchanged), each reading on/off keyed Morse at one audio
 * pitch from one audio row, as characters: a receiver bank's CWU / CWL channels (LINEAR, +-200 Hz, the carrier on a 700 Hz
 * tone) can be decoded in place on its stream after kq_bank_join, and several slots may read one row at different pitches,
 * so that an SSB passband is skimmed with a slot every 100 Hz or so.  The reference has no Morse decoder: the algorithm is
 * defined here.  Everything after the quantiser is exact integer arithmetic, so no result depends on how sums are ordered
 * or how the stream is cut into calls.
 * Per slot, x[n] is its input row; n counts samples since create or kq_cw_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len; frame k is the samples [k B, (k + 1) B).
 *   quantise   as kq_fsk_* / kq_tone_*: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to
 *              nearest even, NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.
 *   table      kq_tone_*'s: C[j] = rint(32767 cos(2 pi j / 1024)) as int16 (kq_cw_get_table).
 *   correlate  inc = rint(pitch 2^32 / Fs) in double, pitch the float of the params (kq_cw_get_inc); ph(n) = (n inc) mod
 *              2^32 -- no oscillator state is carried -- and j = ph(n) >> 22.  Per frame I = sum q[n] C[j], Q = sum q[n]
 *              C[(j - 256) & 1023]: exact integers in 64 bits.  a = I >> 15, b = Q >> 15 (arithmetic shifts), P[k] = a^2 +
 *              b^2 as uint64.  With B <= 4096: |I|, |Q| < 2^42, |a| < 2^27, P < 2^55.
 *   speeds     a dot of w words per minute lasts 1.2 / w seconds, 19.2 Fs / (B w) sixteenths of a frame.  In double, the
 *              speeds the floats of the config and the params: u_min = floor(19.2 Fs / (B max_wpm)), u_max = ceil(19.2 Fs /
 *              (B min_wpm)), and a slot starts at u = rint(19.2 Fs / (B wpm)).
 *   state      hi, lo (uint64), key, cand, run, u (the dot in 1/16 frame), code, nelem, the flags closed and worded, first
 *              and last (frame numbers), frames.  At the set: all zero but u, code = 1, closed = worded = 1.
 *   tracker    one step per completed frame k with P = P[k], in this order (frames += 1 first, saturating):
 *     1 peak      if P > hi: hi = P, else hi -= hi >> 8.
 *     2 validity  valid = frames >= warm and hi >= min_p and hi >= (lo >> 4) snr (snr in sixteenths; < 2^63).
 *     3 threshold d = hi > lo ? hi - lo : 0; thr = lo + (d >> 2) with the key up, lo + (d >> 3) with the key down (half and
 *                 about a third of the amplitude: hysteresis).  lev = valid and P >= thr.
 *     4 floor     if lev == 0, or key == 1 and 16 run > 8 u (a carrier, not keying): lo += (P - lo) >> 5, an arithmetic
 *                 shift of the signed difference.  lo does not follow P through the debounce frames of a rising mark.
 *     5 debounce  if lev == key: run = min(run + 1 + cand, 2^28 - 1), cand = 0 (a glitch shorter than deb is absorbed).
 *                 Else cand += 1, and once cand >= deb the old state closes with length run: a mark is classified (6) and
 *                 last = k + 1 - cand; a space that ends with nelem == 0 sets first = k + 1 - cand.  Then key = lev,
 *                 run = cand, cand = 0.
 *     6 mark      m = 16 run.  m > 8 u: a carrier, code = 0.  m < 2 u: a dot, code = 2 code, u += (m - u) >> 2.  Otherwise a
 *                 dash, code = 2 code + 1 (code 0 stays 0), u += (floor(m / 3) - u) >> 2.  The shifts are arithmetic, on
 *                 signed differences.  Then u is clamped to [u_min, u_max], nelem += 1, code = 0 once nelem > 8, and
 *                 closed = worded = 0.
 *     7 space     with the key up (after step 5, so at the frame where the count is reached, not at the next mark): if not
 *                 closed and 16 run >= 2 u, the character is filed as an event (code, nelem, u, first B, last B, hi) and
 *                 code = 1, nelem = 0, closed = 1.  If not worded and 16 run >= 5 u, a word gap is filed (code 1, nelem 0,
 *                 u, last B, (k + 1) B, hi) and worded = 1.
 *   event      code: the elements behind a leading 1, the first sent in the highest place, dot 0 and dash 1 (A is 0b101);
 *              1: a word gap; 0: undecodable (a mark beyond 8 dots, or a ninth element).  events += 1 for each; it goes to
 *              the slot's arena, or dropped += 1 when that holds max_events.
 * kq_cw_remove and kq_cw_reset discard the open character.  Carried between calls: the open frame's I and Q and the
 * whole tracker state; so the same stream split differently into calls or blocks gives the same events and status.
 * Limits (refused by kq_cw_create / kq_cw_set with the reason in kq_last_error, before any HIP call): samprate positive
 * and finite; 8 <= B <= 4096; 0 < min_wpm <= max_wpm, finite, with u_min >= 48 (three frames in a dot at max_wpm) and
 * u_max <= 2^20; deb 1..16; warm 0..65535; snr 16..4095; min_p <= 2^55; input_scale > 0; max_slots 1..16384; max_events
 * 1..4096; max_samples 1..2^28; per slot 0 < pitch < Fs / 2 and min_wpm <= wpm <= max_wpm.
 * Device memory per slot: 40 max_events of arena, 112 of state and parameters; 2 KiB of table per bank.
 * Copying accuracy on hand-keyed, off-air signals has not been measured; there is no AFC on the pitch (a frame's
 * bandwidth is Fs / B, 250 Hz at 12 kHz and B = 48) and no weighting for hand-sent code.
 * Calls: as kq_fsk_*.  kq_cw_create touches no device. */
typedef struct kq_cw_bank kq_cw_bank;
typedef struct kq_cw_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame */
  float min_wpm, max_wpm;    /* the speeds the tracker may follow */
  unsigned deb;              /* frames a level must last to change the key (2) */
  unsigned warm;             /* frames after the set in which the key is held up while lo trains (64) */
  unsigned snr;              /* least hi / lo, in sixteenths (256: 12 dB) */
  uint64_t min_p;            /* least hi */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_cw_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_cw_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_cw_config;
typedef struct kq_cw_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float pitch;               /* Hz */
  float wpm;                 /* the speed the tracker starts from */
} kq_cw_params;
typedef struct kq_cw_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t key;              /* 1: down */
  uint32_t run;              /* frames in the present state of the key */
  uint32_t unit;             /* u */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t cand;             /* the rest is the open character and the open frame, as carried to the next call */
  uint32_t code;
  uint32_t nelem;
  uint32_t flags;            /* closed | worded << 1 */
  uint64_t hi, lo;           /* peak and floor: of neighbouring slots on one signal the largest hi / lo is on it */
  uint64_t first, last;      /* frame numbers */
  int64_t acc_i, acc_q;      /* I and Q of the open frame */
} kq_cw_status;
typedef struct kq_cw_event {
  uint32_t code;
  uint32_t nelem;
  uint32_t unit;             /* u at the close: the sender's speed is 19.2 Fs / (B unit) WPM */
  uint32_t reserved;         /* 0 */
  uint64_t start_sample;     /* the first mark's first frame, times B (word gap: the last mark's end) */
  uint64_t end_sample;       /* the last mark's end (word gap: the end of the frame that decided it) */
  uint64_t peak;             /* hi at the close */
} kq_cw_event;

kq_cw_bank *kq_cw_create(const kq_cw_config *cfg);
int kq_cw_destroy(kq_cw_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device: the next kq_cw_process, kq_cw_pull_counts or kq_cw_pull_event brings every slot set or removed since
 * the last one there, and waits for the handle's stream to do so (once, however many slots changed). */
int kq_cw_set(kq_cw_bank *bank, unsigned slot, const kq_cw_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_cw_remove(kq_cw_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_fsk_process / kq_tone_process (status may be NULL; nothing is written for an empty
 * slot). */
int kq_cw_process(kq_cw_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                  unsigned nblocks, int on_device, kq_cw_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_cw_pull_counts(kq_cw_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_cw_pull_event(kq_cw_bank *bank, unsigned slot, unsigned index, kq_cw_event *event);
/* Empties every arena (on the handle's stream); the status counters and the open characters go on */
int kq_cw_clear_events(kq_cw_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_cw_get_table(const kq_cw_bank *bank, int16_t *dst, size_t cap);
/* inc of `slot` in *inc; -1 when the slot holds no decoder */
int kq_cw_get_inc(kq_cw_bank *bank, unsigned slot, uint32_t *inc);
int kq_cw_sync(kq_cw_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_cw_reset(kq_cw_bank *bank);

/* --- RTTY (start-stop FSK teleprinter) decoder bank -----------------------------------------------------------------------
 * Up to 16384 decoder slots, each reading two-tone FSK with asynchronous framing (one start bit, 5 to 8 data bits, a stop
 * element) from one audio row, as characters: amateur RTTY (45.45 baud, 170 Hz shift), the weather services' 50 baud with
 * 450 Hz, 75 baud links with 850 Hz.  A receiver bank's USB / LSB channels can be decoded in place on its stream after
 * kq_bank_join, and several slots may read one row at different tone pairs.  The reference has no RTTY decoder: the
 * algorithm is defined here.  Everything after the quantiser is exact integer arithmetic, so no result depends on how sums
 * are ordered or how the stream is cut into calls.
 * Per slot, x[n] is its input row; n counts samples since create or kq_rtty_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise   kq_cw_*'s: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to nearest even,
 *              NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.
 *   table      kq_cw_*'s: C[j] = rint(32767 cos(2 pi j / 1024)) as int16 (kq_rtty_get_table).
 *   correlate  per tone inc = rint(f 2^32 / Fs) in double, f the float of the params (inc_m of mark, inc_s of space:
 *              kq_rtty_get_slot); ph(n) = (n inc) mod 2^32 -- no oscillator state is carried -- and j = ph(n) >> 22.  Per
 *              frame and tone I = sum q[n] C[j], Q = sum q[n] C[(j - 256) & 1023]: exact integers in 64 bits, |I|, |Q| <
 *              2^38.  They are reduced as a = I >> 12, b = Q >> 12 (arithmetic shifts): |a|, |b| < 2^26.
 *   bit        tb = rint(256 Fs / (B baud)) in double, baud the float of the params: the bit in 1/256 frame, 2048 <= tb <=
 *              8192 (8 to 32 frames in a bit).  W = (tb + 128) >> 8 frames, 8..32.
 *   window     per tone SI[k], SQ[k]: the sums of a and b over the frames k - W + 1 .. k, zeros before the set; below 2^31
 *              in magnitude.  Pm = SIm^2 + SQm^2, Ps likewise, as uint64 (below 2^63): a matched filter one bit long, read
 *              out every frame, coherent because the reference phase depends on n alone.
 *   state      sig, nse (uint64), state (0 WAIT, 1 IDLE, 2 CHAR), t (signed, in 1/256 frame), bit, code, start (a frame
 *              number), the counters.  At the set all of it is zero.
 *   step       one per completed frame k, in this order:
 *     1 count     frames += 1, saturating.  hi = max(Pm, Ps), lo = min(Pm, Ps), lev = Pm >= Ps (1 is mark).
 *     2 levels    samp = state == CHAR and t - 256 < 128: this frame samples a bit.  If state != CHAR: sig += (hi - sig)
 *                 >> 6, nse += (lo - nse) >> 6.  If samp: the same with >> 4.  Otherwise (inside a character, between its
 *                 sampling points, where the window straddles two bits) they stand.  Arithmetic shifts of signed
 *                 differences.
 *     3 validity  valid = frames >= warm and sig >= min_p and 16 sig >= nse snr, the products taken exactly (they need up
 *                 to 75 bits: two words).  If not valid: state = WAIT, and the step ends (t, bit, code stand).
 *     4 framer    WAIT: if lev == 1, state = IDLE.
 *                 IDLE: if lev == 0, state = CHAR, t = tb >> 1, bit = -1, code = 0, start = k (the window's output
 *                 crosses half a bit behind the edge and is best a whole bit behind it).
 *                 CHAR: t -= 256; if samp, t += tb and the bit is read: with bit == -1 (the start bit) lev == 1 counts
 *                 false_starts += 1 and state = IDLE, lev == 0 makes bit = 0; with bit < nbits, code |= lev << bit and
 *                 bit += 1 (the first data bit sent is the lowest); with bit == nbits (the stop element, one bit behind
 *                 the last data bit) the character is filed: lev == 1 with flags 0 and state = IDLE, lev == 0 with flags 1
 *                 (framing error), ferr += 1 and state = WAIT, so that a long space (a break) files once.
 *   event      code, flags, start_sample = start B, sig, nse.  events += 1 for each; it goes to the slot's arena, or
 *              dropped += 1 when that holds max_events.  The device hands out raw codes: letters / figures, unshift on
 *              space and the alphabets are the client's (ka9q_sdr_amd/baudot.py).  events, dropped, ferr and false_starts
 *              saturate at 2^32 - 1, as frames does.
 * kq_rtty_remove and kq_rtty_reset discard the open character.  Carried between calls: per tone the open frame's I and Q,
 * the reduced sums of the last 31 frames (W - 1 at the most), the four window sums, and the level and framer state; so the
 * same stream split differently into calls or blocks gives the same events and status.  kq_rtty_status holds all of it but
 * the past frames.
 * A reversed signal is served by swapping mark and space in the params; there is no device flag for it.
 * Limits (refused by kq_rtty_create / kq_rtty_set with the reason in kq_last_error, before any HIP call): samprate positive
 * and finite; 8 <= B <= 256; warm 0..65535; snr 16..4095; min_p <= 2^55; input_scale > 0; max_slots 1..16384; max_events
 * 1..4096; max_samples 1..2^28; per slot 0 < mark, space < Fs / 2, mark != space, nbits 5..8, baud positive and finite
 * with 2048 <= tb <= 8192.
 * Device memory per slot: 32 max_events of arena, 640 of state, history and parameters; 2 KiB of table per bank.
 * Copying off-air signals has not been measured.  There is no AFC on the tone pair, no per-tone threshold correction under
 * selective fading, and a start bit is found from a single frame's level: at an Eb/N0 of 12 dB and below the model loses
 * characters by the tens of per cent.
 * Calls: as kq_cw_*.  kq_rtty_create, kq_rtty_set and kq_rtty_remove touch no device. */
typedef struct kq_rtty_bank kq_rtty_bank;
typedef struct kq_rtty_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which nothing is read while the levels train (64) */
  unsigned snr;              /* least sig / nse, in sixteenths (96: a ratio of 6; noise alone gives about 3) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_rtty_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_rtty_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_rtty_config;
typedef struct kq_rtty_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float mark, space;         /* Hz */
  float baud;
  unsigned nbits;            /* data bits in a character, 5..8 */
} kq_rtty_params;
typedef struct kq_rtty_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t state;            /* 0 WAIT, 1 IDLE, 2 CHAR */
  int32_t bit;               /* the next to be read: -1 the start bit, nbits the stop element */
  uint32_t code;             /* of the open character */
  int32_t t;                 /* 1/256 frame to the next sampling point */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t ferr;             /* characters filed with a framing error */
  uint32_t false_starts;
  uint32_t reserved;         /* 0 */
  uint64_t sig, nse;         /* the levels: of slots on one row the largest sig / nse is on the signal */
  uint64_t start;            /* frame number at which the open (or last) character began */
  int32_t sum_im, sum_qm, sum_is, sum_qs;   /* the window sums at the last completed frame */
  int64_t acc_im, acc_qm, acc_is, acc_qs;   /* I and Q of the open frame */
} kq_rtty_status;
typedef struct kq_rtty_event {
  uint32_t code;
  uint32_t flags;            /* bit 0: framing error (the stop element read space) */
  uint64_t start_sample;     /* the frame at which the start bit was seen, times B: half a bit behind its edge */
  uint64_t sig, nse;         /* the levels at the stop element */
} kq_rtty_event;
typedef struct kq_rtty_slot {
  uint32_t inc_m, inc_s;     /* the phase increments of mark and space */
  uint32_t tb;               /* the bit in 1/256 frame */
  uint32_t W;                /* the window in frames */
} kq_rtty_slot;

kq_rtty_bank *kq_rtty_create(const kq_rtty_config *cfg);
int kq_rtty_destroy(kq_rtty_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device: the next kq_rtty_process, kq_rtty_pull_counts or kq_rtty_pull_event brings every slot set or removed
 * since the last one there, and waits for the handle's stream to do so (once, however many slots changed). */
int kq_rtty_set(kq_rtty_bank *bank, unsigned slot, const kq_rtty_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_rtty_remove(kq_rtty_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_cw_process (status may be NULL; nothing is written for an empty slot). */
int kq_rtty_process(kq_rtty_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                    unsigned nblocks, int on_device, kq_rtty_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_rtty_pull_counts(kq_rtty_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_rtty_pull_event(kq_rtty_bank *bank, unsigned slot, unsigned index, kq_rtty_event *event);
/* Empties every arena (on the handle's stream); the status counters and the open characters go on */
int kq_rtty_clear_events(kq_rtty_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_rtty_get_table(const kq_rtty_bank *bank, int16_t *dst, size_t cap);
/* inc_m, inc_s, tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_rtty_get_slot(kq_rtty_bank *bank, unsigned slot, kq_rtty_slot *out);
int kq_rtty_sync(kq_rtty_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_rtty_reset(kq_rtty_bank *bank);

/* --- PSK31 / PSK63 / PSK125 decoder bank ------------------------------------------------------------------------------------
 * Up to 16384 decoder slots, each reading differential BPSK with Varicode framing (PSK31 at 31.25 baud and its faster
 * siblings at 62.5 and 125) at one audio pitch from one audio row, as characters.  A receiver bank's USB / LSB channels can
 * be decoded in place on its stream after kq_bank_join, and several slots may read one row at different pitches, so that a
 * 3 kHz passband is skimmed with a slot every 50 Hz or so.  The reference has no PSK decoder: the algorithm is defined
 * here.  Everything after the quantiser is exact integer arithmetic, so no result depends on how sums are ordered or how
 * the stream is cut into calls.
 * Per slot, x[n] is its input row; n counts samples since create or kq_psk_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise   kq_cw_*'s: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to nearest even,
 *              NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.
 *   table      kq_cw_*'s: C[j] = rint(32767 cos(2 pi j / 1024)) as int16 (kq_psk_get_table).
 *   correlate  inc = rint(pitch 2^32 / Fs) in double, pitch the float of the params (kq_psk_get_slot); ph(n) = (n inc) mod
 *              2^32 -- no oscillator state is carried -- and j = ph(n) >> 22.  Per frame I = sum q[n] C[j], Q = sum q[n]
 *              C[(j - 256) & 1023]: exact integers in 64 bits, |I|, |Q| <= 256 * 32767^2 < 2^38.  They are reduced as a =
 *              I >> 13, b = Q >> 13 (arithmetic shifts): |a|, |b| < 2^25.  A signal above the pitch turns (I, Q) clockwise.
 *   symbol     tb = rint(256 Fs / (B baud)) in double, baud the float of the params: the symbol in 1/256 frame, 2048 <= tb
 *              <= 8192 (8 to 32 frames in a symbol).  W = (tb + 128) >> 8 frames, 8..32.  q = tb >> 2, a quarter symbol.
 *   window     SI[k], SQ[k]: the sums of a and b over the frames k - W + 1 .. k, zeros before the set; 32 terms at the
 *              most, so below 2^30 in magnitude.  P = SI^2 + SQ^2 as uint64, below 2^61.  The window is a rectangle one
 *              symbol long, coherent because the reference phase depends on n alone.  It is not the matched filter of
 *              PSK31's cosine-shaped symbols.
 *   state      frames, ph (0 early, 1 centre, 2 late: the point taken next), t (signed, in 1/256 frame, to that point),
 *              pe, ee, el (early and late power, the last and the smoothed two), c and p (the window sums at this
 *              symbol's centre and at the one before), pc, R = (rot_r, rot_i) (the smoothed product of neighbouring
 *              symbols: the turn per symbol that a frequency offset makes), sig, qre, qim, shreg, over, the counters.  At
 *              the set all of it is zero.
 *   step       one per completed frame k: frames += 1, saturating; t -= 256.  If t >= 128 nothing more happens in this
 *              frame.  Otherwise the frame is a point, taken in turn by ph:
 *                early   pe = P, t += q, ph = 1.
 *                centre  c = (SI, SQ), pc = P, t += q, ph = 2.
 *                late    ph = 0, and with pl = P the symbol is read, in this order:
 *     1 timing    ee += (pe - ee) >> 3, el += (pl - el) >> 3 (arithmetic shifts of signed differences, here and below; every
 *                 term is below 2^61).  m = max(ee, el).  adj = -(tb >> 5) if ee > el and ee - el > (m >> 3), +(tb >> 5) if
 *                 el > ee and el - ee > (m >> 3), else 0.  t += tb - 2 q + adj.  The powers are smoothed over symbols so
 *                 that a reversal on one side of a symbol only does not pull the clock.
 *     2 product   D = c conj(p): Dr = cr pr + ci pi, Di = ci pr - cr pi, each two products below 2^60, so below 2^61 in
 *                 magnitude.  Then p = c.
 *     3 normalise norm(x, y): s = max(bitlength(max(|x|, |y|)) - 24, 0), giving (x >> s, y >> s), both 2^24 at the most in
 *                 magnitude (arithmetic shifts: only -2^24 itself comes out that large).  d = norm(D); r = norm(R), or
 *                 (1, 0) while R is (0, 0).
 *     4 decision  Re = dr rr + di ri, Im = di rr - dr ri: 2^49 at the most.  bit = Re >= 0.  No reversal is a 1.
 *     5 rotation  D' = bit ? D : -D.  R += (D' - R) >> 4 per component: |D' - R| < 2^62, and |R| stays below 2^61 as D does.
 *                 Then, if 2 rot_r < |rot_i|: rot_r = |rot_i| >> 1.  The estimate stays within atan 2 = 63.4 degrees per
 *                 symbol, which is +-5.5 Hz at 31.25 baud; without the clamp it can settle half a turn off after a stretch
 *                 of noise and invert every bit from there on.
 *     6 levels    qre += (|Re| - qre) >> 4, qim += (|Im| - qim) >> 4, sig += (pc - sig) >> 4.
 *     7 validity  valid = frames >= warm and sig >= min_p and 16 qre >= snr qim (16 qre <= 2^53, snr qim < 2^61: one word).
 *                 If not valid: shreg = 0, over = 0, and the step ends.
 *     8 Varicode  over = 1 if bit 13 of shreg is set; shreg = (shreg << 1 | bit) & 0x3FFF.  If (shreg & 3) == 0 (a gap of
 *                 two reversals): code = shreg >> 2, and when code != 0 an event is filed with flags = over, or flags = 1
 *                 if code > 1023 (more than ten bits between gaps: no character); then shreg = 0, over = 0.
 *   event      code: the character's bits behind their own leading 1, as sent, the first in the highest place (e is 0b11,
 *              a space 0b1: ka9q_sdr_amd/varicode.py holds the table); flags; end_sample = (k + 1) B, the end of the frame
 *              that read the second reversal of the gap; sig; rot_r, rot_i = r of step 3 as int32: the turn per symbol
 *              the decision was made against, -atan2(rot_i, rot_r) / (2 pi) baud Hz above the pitch.  events += 1 for
 *              each; it goes to the slot's arena, or dropped += 1 when that holds max_events.  events and dropped saturate
 *              at 2^32 - 1, as frames does.
 * kq_psk_remove and kq_psk_reset discard the open character.  Carried between calls: the open frame's I and Q, the reduced
 * sums of the last 31 frames (W - 1 at the most), the two window sums and all of the state above; so the same stream split
 * differently into calls or blocks gives the same events and status.  kq_psk_status holds all of it but the past frames.
 * The code is differential, so the carrier's phase and the signal's polarity change nothing.
 * Limits (refused by kq_psk_create / kq_psk_set with the reason in kq_last_error, before any HIP call): samprate positive
 * and finite; 8 <= B <= 256; warm 0..65535; snr 16..4095; min_p <= 2^55; input_scale > 0; max_slots 1..16384; max_events
 * 1..4096; max_samples 1..2^28; per slot 0 < pitch < Fs / 2, baud positive and finite with 2048 <= tb <= 8192.
 * Device memory per slot: 32 max_events of arena, 416 of state, history and parameters; 2 KiB of table per bank.
 * Absent: QPSK31 (its convolutional code needs a Viterbi decoder: a later bank) and a matched filter.  The rectangular
 * window keeps the eye open -- at the centre it reads an amplitude of 0.64 where both neighbours are reversals, 0.82
 * with one, 1.0 with none -- at a cost in noise margin.  The rotation estimate follows +-5.5 Hz at 31.25 baud and no
 * more; the clock tolerates the 100 ppm of a sound card.  There is no squelch beyond step 7: when a signal stops, the
 * gate takes a few symbols to shut, and a slot 50 Hz beside a strong signal reads its splatter as a few characters (of
 * neighbouring slots the largest qre / qim is on the signal).  Copy off the air has not been measured.  In the model
 * (tests/test_psk_model.py), at (12000, 24, 31.25) with snr = 32 and white noise, five runs of 171 characters each are
 * whole at an Es/N0 (the carrier's power times the symbol over N0) of 20 and 14 dB; 0.7 % of the characters are lost at
 * 12 dB, 19 % at 10 dB and 77 % at 8 dB, where the validity gate is shut most of the time.
 * Calls: as kq_rtty_*.  kq_psk_create, kq_psk_set and kq_psk_remove touch no device. */
typedef struct kq_psk_bank kq_psk_bank;
typedef struct kq_psk_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which nothing is read while the levels train (64) */
  unsigned snr;              /* least qre / qim, in sixteenths (32: a ratio of 2; noise alone gives about 1) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_psk_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_psk_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_psk_config;
typedef struct kq_psk_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float pitch;               /* Hz */
  float baud;
} kq_psk_params;
typedef struct kq_psk_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t ph;               /* the point taken next: 0 early, 1 centre, 2 late */
  int32_t t;                 /* 1/256 frame to that point */
  uint32_t shreg;            /* the open character's bits */
  uint32_t over;             /* 1: a set bit has left shreg */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t reserved;         /* 0 */
  uint64_t sig;              /* the power at the symbols' centres */
  uint64_t qre, qim;         /* the decision's |Re| and |Im|: of slots on one row the largest qre / qim is on the signal */
  uint64_t ee, el;           /* the smoothed early and late power */
  uint64_t pe, pc;           /* the power at the last early point and the last centre */
  int64_t rot_r, rot_i;      /* R */
  int32_t cr, ci, pr, pi;    /* c and p */
  int32_t sum_i, sum_q;      /* the window sums at the last completed frame */
  int64_t acc_i, acc_q;      /* I and Q of the open frame */
} kq_psk_status;
typedef struct kq_psk_event {
  uint32_t code;
  uint32_t flags;            /* bit 0: more than ten bits between gaps, code holds the last of them */
  uint64_t end_sample;       /* the end of the frame that read the gap */
  uint64_t sig;              /* at that symbol */
  int32_t rot_r, rot_i;      /* r at that symbol */
} kq_psk_event;
typedef struct kq_psk_slot {
  uint32_t inc;              /* the phase increment of the pitch */
  uint32_t tb;               /* the symbol in 1/256 frame */
  uint32_t W;                /* the window in frames */
  uint32_t reserved;         /* 0 */
} kq_psk_slot;

kq_psk_bank *kq_psk_create(const kq_psk_config *cfg);
int kq_psk_destroy(kq_psk_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device: the next kq_psk_process, kq_psk_pull_counts or kq_psk_pull_event brings every slot set or removed
 * since the last one there, and waits for the handle's stream to do so (once, however many slots changed). */
int kq_psk_set(kq_psk_bank *bank, unsigned slot, const kq_psk_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_psk_remove(kq_psk_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_rtty_process (status may be NULL; nothing is written for an empty slot). */
int kq_psk_process(kq_psk_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_psk_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_psk_pull_counts(kq_psk_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_psk_pull_event(kq_psk_bank *bank, unsigned slot, unsigned index, kq_psk_event *event);
/* Empties every arena (on the handle's stream); the status counters and the open characters go on */
int kq_psk_clear_events(kq_psk_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_psk_get_table(const kq_psk_bank *bank, int16_t *dst, size_t cap);
/* inc, tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_psk_get_slot(kq_psk_bank *bank, unsigned slot, kq_psk_slot *out);
int kq_psk_sync(kq_psk_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_psk_reset(kq_psk_bank *bank);

/* --- ACARS decoder bank -------------------------------------------------------------------------------------------------------
 * Up to 4096 decoder slots, each reading ACARS blocks from the audio of one AM channel (demod_am's output; a receiver
 * bank's audio plane can be decoded in place on its stream after kq_bank_join), so that an airband bank of 760 channels
 * hands out blocks instead of 760 audio streams.  ACARS is 2400 bit/s MSK: a bit equal to the one before is 2400 Hz, one
 * that differs 1200 Hz, the phase continuous -- MSK around 1800 Hz, precoded so that a coherent detector's decisions are
 * the data bits.  A block: a pre-key of 2400 Hz; + * SYN SYN SOH (0x2b 0x2a 0x16 0x16 0x01); mode, address (7), ack,
 * label (2), block id; STX and up to 220 characters of text, or neither; ETX (0x03) or ETB (0x17); the block check, 2 bytes,
 * low first; DEL.  Characters are 7 bits, least significant first, bit 7 making the parity odd.  The check is
 * CRC-16/KERMIT (0x8408 reflected, initial value 0, no final xor) over the bytes as sent, parity bits included, from mode
 * through ETX / ETB; run on over the two check bytes it leaves 0.  This is ARINC 618's block as the open decoders read it,
 * written down from memory: nothing here has been checked against a signal off the air.  The reference has no ACARS
 * decoder: the algorithm is defined here.  Everything after the quantiser is exact integer arithmetic, so no result depends
 * on how sums are ordered or how the stream is cut into calls.
 * Per slot, x[n] is its input row; n counts samples since create or kq_acars_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate.  Integers made from Fs in double, rint to nearest even: FL = rint(2 Fs /
 * 2400) taps (8..80), w = ceil(Fs / 2400) (4..40), e = max(1, rint(Fs / 9600)) (1..10, e <= w), tb = rint(256 Fs / 2400),
 * o_k = rint((k - 39) Fs / 2400) for k = 0..39 (o_39 = 0, H39 = -o_0 <= 1560), inc = rint(1800 2^32 / Fs).
 *   quantise   as kq_fsk_*: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to nearest even,
 *              NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.  |q| < 2^15.
 *   mix        kq_cw_*'s table C[j] = rint(32767 cos(2 pi j / 1024)); j = ((n inc) mod 2^32) >> 22 -- no oscillator state
 *              is carried and nothing feeds back -- and z[n] = q[n] (C[j] - i C[(j - 256) & 1023]).  |Re z|, |Im z| <= 32767^2
 *              < 2^30.
 *   filter     hq[i] = rint(32767 cos(pi (i - (FL - 1) / 2) / FL)) as int16 (kq_acars_get_taps): the half cosine two bits
 *              long, MSK's matched filter.  v[n] = sum_i hq[i] z[n - i], exact in 64 bits: each component is at most
 *              80 * 32767^3 < 2^51.33.  a[n] = v[n] >> 30 per component (arithmetic shift): below 2^21.33, an int32.
 *   sync       d_k = +-1: the 40 bits of + * SYN SYN SOH, parity bits included, in the order sent.  c[n] = sum_k d_k
 *              (-i)^k a[n + o_k] (the correlation against d_k i^k, one bit apart): a component is 40 terms, below 2^26.66.
 *              e[n] = sum_k |a[n + o_k]|^2 < 40 * 2 * 2^42.66 < 2^49.  |c|^2 as uint64 < 2^54.4.  The metric |c|^2 / (40 e)
 *              is 1 at the most.  n passes when |c|^2 > 0 and |c|^2 sync_den >= 40 sync_num e (both sides below 2^62.4:
 *              sync_den <= 255).  p is a sync when it passes, |c[p]|^2 > |c[m]|^2 for p - w <= m < p and |c[p]|^2 >=
 *              |c[m]|^2 for p < m <= p + w (of equals the first), p >= search_from, and no block is open.  It is decided
 *              when sample p + w has arrived, however the stream is cut.
 *              At a sync: syncs += 1; R = (Re c >> 5, Im c >> 5) (below 2^21.66: the sign of the audio is inside, so no
 *              polarity is left to resolve); t = 256 p (in 1/256 sample); k = 39; sync_sample = p, sync_c2 = |c|^2, sync_e =
 *              e; nbits, cur, length, parity_errors, crc, ending, cnt, acc = 0.  p lies (FL - 1) / 2 samples -- the
 *              filter's delay -- behind the end of SOH's last bit.
 *   bit        while a block is open, in order, each when sample n + w has arrived: n = (t + tb + 128) >> 8; t += tb;
 *              k += 1 (mod 2^32); u = a[n] (-i)^(k mod 4), ue and ul the same of a[n - e] and a[n + e].  With <x, R> = Re x
 *              Re R + Im x Im R (below 2^44.1): bit = <u, R> >= 0.  acc += |<ue, R>| - |<ul, R>|.  Then R += (u - R) >> 4 per
 *              component if bit else (-u - R) >> 4 (arithmetic; R stays below 2^22).  cnt += 1; at cnt == 8, with r2 =
 *              |R|^2 of the new R (< 2^44.4): t -= tb >> 5 if 4 acc > r2, t += tb >> 5 if 4 acc < -r2 (|acc| < 2^48); acc =
 *              cnt = 0.  The early / late difference over 8 bits moves the clock when it exceeds a quarter of |R|.
 *   frame      the bit goes into cur at place nbits and into crc (crc = (crc >> 1) ^ (0x8408 if (crc ^ bit) & 1)); at the
 *              8th, the byte is stored behind the others (from the mode character on: length += 1).  If ending != 0 (bytes
 *              of the check left, + 4 behind an ETB): ending -= 1 and at (ending & 3) == 0 the block closes, good when crc
 *              == 0.  Else: parity_errors += 1 for a byte of even parity; a byte with (byte & 0x7f) ETX or ETB and length
 *              <= max_block_bytes - 2 sets ending = 2 (ETB: 6); else, when length >= max_block_bytes - 2, the block closes
 *              as an overrun.
 *   close      at the bit's sample n: blocks_good, overruns or blocks_bad += 1.  A good block, or any other with
 *              parity_errors <= max_parity_errors (so that the host can repair it), goes to the slot's arena, or dropped
 *              += 1 when that holds max_blocks; the rest: discarded += 1.  Then in_block = 0, ending = 0, search_from =
 *              n + 1: the search goes on behind the block's last bit (DEL is not read).  Counters saturate at 2^32 - 1.
 *   record     the bytes from mode through the check, parity bits kept; length; flags (KQ_ACARS_GOOD, KQ_ACARS_ETB,
 *              KQ_ACARS_OVERRUN); parity_errors; sync_sample; end_sample = n of the last bit; sync_c2 and sync_e (the metric is
 *              sync_c2 / (40 sync_e)); r2 = |R|^2 at the close.
 * A call's results look back on the H = H39 + 2 w + FL - 1 samples before it (1719 at the most; 214 at 12 kHz).  Carried
 * between calls, in the form the next call needs them: the last FL - 1 values of q, the last HA = H39 + 2 w values of a, the
 * last 2 w of |c|^2 with the threshold's verdict -- each a function of the samples alone -- kq_acars_status, which is all
 * of the state above, and the open block's bytes.  So the same stream cut differently into calls or blocks gives the same
 * records and status.
 * Limits (refused by kq_acars_create / kq_acars_set with the reason in kq_last_error, before any HIP call): samprate finite,
 * 9600 <= Fs <= 96000 (4 to 40 samples per bit); input_scale > 0; sync_den 1..255, sync_num 1..sync_den; max_parity_errors
 * 0..255; max_block_bytes 16..256; max_slots 1..4096; max_blocks 1..4096; max_samples 1..2^28.
 * Device memory per slot: 8 HA + 16 w + 4 (FL - 1) bytes of the past (13.9 KiB at 96 kHz, 1.7 KiB at 12 kHz), 256 of open
 * block, max_blocks (max_block_bytes + 56) of arena, 128 of state and parameters; 2.5 KiB of tables per bank.
 * Absent: a squelch other than the metric; soft decisions; the reading of DEL; anything above the block (multi-block
 * messages are the host's: ka9q_sdr_amd/arinc618.py parses and repairs).  In the model (tests/test_acars_model.py), at 12
 * kHz with white noise, five runs of ten blocks each are whole at an Eb/N0 of 14 and 10 dB; at 8 dB 39 are good and 11
 * repairable, at 6 dB 5 good, 27 repairable and 18 lost.  120 s of noise alone and of a steady 2400 Hz tone file nothing and
 * never pass the threshold (metric 0.27 and 0.18 at the most against 0.5).
 * Calls: as kq_psk_*.  kq_acars_create, kq_acars_set and kq_acars_remove touch no device. */
#define KQ_ACARS_GOOD 1u     /* the check closed */
#define KQ_ACARS_ETB 2u      /* ended by ETB: another block of the message follows */
#define KQ_ACARS_OVERRUN 4u  /* max_block_bytes passed without ETX / ETB */
typedef struct kq_acars_bank kq_acars_bank;
typedef struct kq_acars_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned sync_num, sync_den; /* the sync threshold on |c|^2 / (40 e): 1 / 2 */
  unsigned max_parity_errors; /* a block whose check fails is filed with this many at the most (3) */
  unsigned max_block_bytes;  /* longest block, check included (256) */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 4096) */
  unsigned max_blocks;       /* arena places per slot between kq_acars_clear_blocks calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_acars_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_acars_config;
typedef struct kq_acars_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
} kq_acars_params;
typedef struct kq_acars_status {
  uint32_t syncs;            /* since the slot was set, as the counters below */
  uint32_t blocks_good, blocks_bad, overruns;   /* closed: check good, check bad, no ETX / ETB */
  uint32_t dropped;          /* refused by a full arena */
  uint32_t discarded;        /* bad or overrun with more than max_parity_errors: counted only */
  uint32_t in_block;         /* 1: a block is open */
  uint32_t k;                /* bits since the sync's first, mod 2^32 */
  uint32_t nbits, cur;       /* the open character */
  uint32_t length;           /* bytes of the open block */
  uint32_t parity_errors;
  uint32_t crc;
  uint32_t ending;           /* bytes of the check left, + 4 behind an ETB */
  uint32_t cnt;              /* bits gathered in acc */
  uint32_t reserved;         /* 0 */
  int64_t t;                 /* the last bit's time, 1/256 sample */
  int64_t search_from;       /* no sync before this sample */
  int64_t acc;               /* early minus late */
  uint64_t sync_sample, sync_c2, sync_e;   /* of the last sync */
  int32_t rr, ri;            /* R */
} kq_acars_status;
typedef struct kq_acars_block_info {
  uint32_t length;
  uint32_t flags;            /* KQ_ACARS_* */
  uint32_t parity_errors;
  uint32_t reserved;         /* 0 */
  uint64_t sync_sample, end_sample;
  uint64_t sync_c2, sync_e;
  uint64_t r2;
} kq_acars_block_info;
typedef struct kq_acars_slot {
  uint32_t source;
  uint32_t inc;              /* the mixer's phase increment */
  uint32_t taps;             /* FL */
  uint32_t w, e, tb;
  uint32_t history;          /* H: the samples before a call that its results look back on */
  uint32_t piece;            /* samples the kernel takes through LDS at a time (a seam for call splits) */
} kq_acars_slot;

kq_acars_bank *kq_acars_create(const kq_acars_config *cfg);
int kq_acars_destroy(kq_acars_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device, as kq_psk_set */
int kq_acars_set(kq_acars_bank *bank, unsigned slot, const kq_acars_params *params);
/* The slot stops from the next call and its open block is discarded; its arena stays readable.  Touches no device either */
int kq_acars_remove(kq_acars_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_fsk_process (status may be NULL; nothing is written for an empty slot). */
int kq_acars_process(kq_acars_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                     unsigned nblocks, int on_device, kq_acars_status *status, size_t status_stride);
/* Blocks in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_acars_pull_counts(kq_acars_bank *bank, uint32_t *counts);
/* Copies block `index` of `slot` (at most cap bytes) and its record (info may be NULL); returns its length, or -1 */
int kq_acars_pull_block(kq_acars_bank *bank, unsigned slot, unsigned index, unsigned char *dst, size_t cap,
                        kq_acars_block_info *info);
/* Empties every arena (on the handle's stream); the status counters and the open blocks go on */
int kq_acars_clear_blocks(kq_acars_bank *bank);
/* hq (at most cap words); returns FL */
int kq_acars_get_taps(const kq_acars_bank *bank, int16_t *dst, size_t cap);
/* the slot's source and the bank's integers, without a device; -1 when the slot holds no decoder */
int kq_acars_get_slot(kq_acars_bank *bank, unsigned slot, kq_acars_slot *out);
int kq_acars_sync(kq_acars_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_acars_reset(kq_acars_bank *bank);

/* --- HF ALE (MIL-STD-188-141 Appendix A, 8-FSK) decoder bank ------------------------------------------------------------------
 * Up to 16384 decoder slots, each reading second-generation Automatic Link Establishment words from one audio row: a
 * receiver bank with a USB channel parked on every ALE frequency, and a slot on each, hears every sounding and call.  A
 * bank's USB channels can be decoded in place on its stream after kq_bank_join.  The reference has no ALE decoder: the
 * algorithm is defined here.  Everything after the quantiser is exact integer arithmetic, so no result depends on how sums
 * are ordered or how the stream is cut into calls.
 * The signal, WRITTEN DOWN FROM MEMORY (no copy of the standard was at hand; ka9q_sdr_amd/ale2g.py says the same): eight
 * tones at 750 + 250 t Hz, t = 0..7, phase-continuous, 125 symbols a second, three bits a symbol with the highest sent
 * first; the tones 0..7 carry 000 001 011 010 110 111 101 100.  A word is 24 bits, highest first: a 3-bit preamble (DATA 0,
 * THRU 1, TO 2, TWAS 3, FROM 4, TIS 5, CMD 6, REP 7) and three 7-bit ASCII characters, in addresses from the 38 of 0-9 A-Z
 * @ ?.  Its halves A (bits 23..12) and B (bits 11..0) are each encoded with the extended Golay (24,12,8) code, 12 data bits
 * then 12 check bits, B's check bits inverted; A23 B23 A22 B22 .. A0 B0 and one stuff bit 0 make 49 bits, which are sent
 * three times in a row: 147 bits, 49 symbols, 392 ms.  The check bits here are the remainder of data x^11 by g(x) = x^11 +
 * x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75) followed by the overall parity bit.  That this is a (24,12,8) code whose 2325
 * error patterns of weight <= 3 have distinct syndromes is tested; that it equals the standard's generator matrix bit for
 * bit is NOT verified.  The 4096-entry parity table (ale2g.PARITY, golay_parity() in kq_ale.hip) is the single statement of
 * the code, so a correction is a table swap.
 * Per slot, x[n] is its input row; n counts samples since create or kq_ale_reset on a grid shared by every slot, and x[n] = 0
 * before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise   kq_cw_*'s: q[n] = clamp(rint(x[n] input_scale), -32767, 32767), one float multiply, round to nearest even,
 *              NaN reads as 0; a KQ_PCM_S16BE word is taken as q itself, -32768 as -32767.
 *   table      kq_cw_*'s: C[j] = rint(32767 cos(2 pi j / 1024)) as int16 (kq_ale_get_table).
 *   correlate  tone t is at f0 + t df in double, f0 and df the floats of the params; inc[t] = rint((f0 + t df) 2^32 / Fs)
 *              (kq_ale_get_slot); ph_t(n) = (n inc[t]) mod 2^32 -- no oscillator state is carried -- and j = ph_t(n) >> 22.
 *              Per frame and tone I = sum q[n] C[j], Q = sum q[n] C[(j - 256) & 1023]: exact integers in 64 bits.  The
 *              vector (I, Q) is at most 256 * 32767 * 32768 < 2^38 long (a table entry's pair is at most 32767.8 long).
 *              Reduced as kq_rtty_* does: a = I >> 12, b = Q >> 12 (arithmetic shifts), (a, b) at most 2^26 + 2 long.
 *   symbol     tb = rint(256 Fs / (B baud)) in double, baud the float of the params: the symbol in 1/256 frame, 2048 <= tb
 *              <= 8192 (8 to 32 frames in a symbol).  W = (tb + 128) >> 8 frames, 8..32.  q = tb >> 2, a quarter symbol.
 *   window     per tone SI_t[k], SQ_t[k]: the sums of a and b over the frames k - W + 1 .. k, zeros before the set; 32 terms
 *              at the most, so each fits int32 and the vector is at most 2^31 + 64 long.  P_t = SI_t^2 + SQ_t^2 as uint64,
 *              below 2^63.  The tones are orthogonal over a symbol, so this is the matched filter.  best = max P_t, sym =
 *              the lowest t that has it, oth = the sum over the other seven t of (P_t >> 3), below 2^63: seven eighths of
 *              the mean of the other seven, taken so that no sum passes 64 bits and no division is needed.
 *   state      frames, ph (0 early, 1 centre, 2 late: the point taken next), t (signed, in 1/256 frame, to that point), pe,
 *              ee, el (early and late power, the last and the smoothed two), sym, pc and oth (of the last centre), sig, nse,
 *              the register r0, r1, r2 (49 bits each), nsym, sync_at, wpos, synced, bad, the counters.  At the set all zero.
 *   step       one per completed frame k: frames += 1, saturating; t -= 256.  If t >= 128 nothing more happens in this
 *              frame.  Otherwise the frame is a point, taken in turn by ph:
 *                early   pe = best, t += q, ph = 1.
 *                centre  sym, pc = best and oth are taken, t += q, ph = 2.
 *                late    ph = 0, and with pl = best the symbol is read, in this order:
 *     1 timing    kq_psk_*'s: ee += (pe - ee) >> 3, el += (pl - el) >> 3 (arithmetic shifts of signed differences, here and
 *                 below; every term is below 2^63).  m = max(ee, el).  adj = -(tb >> 5) if ee > el and ee - el > (m >> 3),
 *                 +(tb >> 5) if el > ee and el - ee > (m >> 3), else 0.  t += tb - 2 q + adj.  Where neighbouring symbols
 *                 carry the same tone both sides read alike and the clock holds.
 *     2 levels    sig += (pc - sig) >> 4, nse += (oth - nse) >> 4.  valid = frames >= warm and sig >= min_p and 16 sig >= snr
 *                 nse, the two products taken exactly (they pass 64 bits: 128-bit compare).
 *     3 register  g = the three bits of tone sym.  r0 = (r0 << 3 | r1 >> 46) mod 2^49, r1 = (r1 << 3 | r2 >> 46) mod 2^49,
 *                 r2 = (r2 << 3 | g) mod 2^49, each from the values before.  nsym += 1 (mod 2^32); if synced, wpos += 1.
 *     4 gate      if not valid: synced = 0, bad = 0, wpos = 0, and the step ends: the register has shifted all the same.
 *     5 word      if synced and wpos < 49 the step ends.  Otherwise the attempt: maj = (r0 & r1) | (r0 & r2) | (r1 & r2);
 *                 split = popcount((r0 ^ r1) | (r0 ^ r2)), the places where the copies differ; A = bits 48, 46 .. 2 of maj
 *                 and B = bits 47, 45 .. 1, the first named in bit 23; B ^= 0xFFF; per half the syndrome = parity[half >> 12]
 *                 ^ (half & 0xFFF), and by a second 4096-entry table the one error pattern of weight <= 3 with that
 *                 syndrome, or weight 4 where there is none (1771 of 4096 syndromes).  err_a, err_b = the weights; word =
 *                 A's and B's data bits, corrected where the weight is below 4, as received where it is 4.
 *                   not synced  The word is filed (flags 0) only if err_a <= acq_err and err_b <= acq_err, bit 0 of maj
 *                               (the stuff bit) is 0, and -- for every preamble but CMD -- all three characters are among
 *                               the 38.  Then synced = 1, sync_at = nsym, wpos = 0, bad = 0.
 *                   synced      wpos = 0.  If both weights are below 4 the word is filed (flags 0) with no further test and
 *                               bad = 0.  Otherwise it is filed with flags bit 0 set, so that the client sees the hole;
 *                               bad += 1, and at bad == lose: synced = 0, bad = 0.
 *                 2325 / 4096 of all 24-bit words lie within three bits of a codeword, so a search at every symbol must
 *                 not use the code's full reach: with acq_err = 1 a random half passes with probability 25 / 4096, a random
 *                 147 bits with (25 / 4096)^2 / 2 and, outside CMD, (38 / 128)^3 of that.
 *   event      word (24 bits); flags; err_a, err_b; split; end_sample = (k + 1) B, the end of the frame of the late point
 *              that read the word's last symbol; sig, nse at that symbol.  events += 1 for each; it goes to the slot's
 *              arena, or dropped += 1 when that holds max_events.  events and dropped saturate at 2^32 - 1, as frames.
 * A departure from word sync by counting: (nsym - sync_at) mod 49 == 0 is kept as wpos, which counts 0..49 and does not
 * mind nsym wrapping.  kq_ale_remove and kq_ale_reset discard the register.  Carried between calls: the open frame's I and Q
 * per tone, the reduced sums of the last 31 frames (W - 1 at the most), the sixteen window sums and all of the state above;
 * so the same stream split differently into calls or blocks gives the same events and status.  kq_ale_status holds all of
 * it but the past frames.
 * Limits (refused by kq_ale_create / kq_ale_set with the reason in kq_last_error, before any HIP call): samprate positive
 * and finite; 8 <= B <= 256; warm 0..65535; snr 16..4095; min_p <= 2^55; input_scale > 0; acq_err 0..3; lose 1..15;
 * max_slots 1..16384; max_events 1..4096; max_samples 1..2^28; per slot f0 and df finite, df not 0 (it may be negative: an
 * LSB channel), every tone above 0 and below Fs / 2, baud positive and finite with 2048 <= tb <= 8192.
 * Device memory per slot: 48 max_events of arena, about 2.4 KiB of state, history and parameters; 18 KiB of tables per bank.
 * The default snr of 80 (sig / nse = 5): in the model 60 s of noise alone hold 16 sig / nse between 56 and 82, mean 66 (the
 * largest of eight noise powers is about 3.6 times the mean of the other seven, and nse is 7 / 8 of that mean), a signal
 * at an Es/N0 of 6 dB between 79 and 122, at 8 dB between 112 and 158.  The gate is a squelch only: noise and a steady tone
 * file nothing with the gate held open either, by the code and the character test alone (tests/test_ale_model.py).  So a
 * gate that opens on noise costs nothing but the attempts, while one that shuts on a weak signal costs words: 80 is the
 * top of what noise reaches (it is valid at 101 of 7497 symbols of noise), not the middle between noise and signal.  When
 * a signal ends in silence sig and nse fall together and the gate stays open until sig < min_p; in noise it shuts.
 * Absent: soft decisions, a per-tone fading correction, any AFC beyond what f0 is set to, the AMD / DTM / DBM message
 * protocols above the word, 3G ALE.  It has not met a signal off the air, and until it has, the Golay table above stands
 * unverified against the standard.  In the model, at (8000, 8) and (39062.5, 32) with white noise, four runs of 16 random
 * words behind four lead-in words are whole at an Es/N0 (a tone's power times the symbol over N0) of 20, 14, 12, 10 and 8
 * dB (64 of 64 at both geometries); at 6 dB 27 and 32 of 64 are read, and one word at each is read wrong (in word sync a
 * half is taken with up to three corrections).  Measured on the integer model on a CPU; the kernel equals it bit for bit.
 * Calls: as kq_psk_*.  kq_ale_create, kq_ale_set and kq_ale_remove touch no device. */
typedef struct kq_ale_bank kq_ale_bank;
typedef struct kq_ale_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which nothing is read while the levels train (64) */
  unsigned snr;              /* least sig / nse, in sixteenths (80; noise alone gives about 66) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_ale_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_ale_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
  unsigned acq_err;          /* most bits corrected per Golay half to accept a word while not in word sync, 0..3 (1) */
  unsigned lose;             /* failed words in a row that end word sync, 1..15 (2) */
} kq_ale_config;
typedef struct kq_ale_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float f0;                  /* Hz, tone 0 (750) */
  float df;                  /* Hz between tones (250; negative on an LSB channel) */
  float baud;                /* 125 */
} kq_ale_params;
typedef struct kq_ale_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t ph;               /* the point taken next: 0 early, 1 centre, 2 late */
  int32_t t;                 /* 1/256 frame to that point */
  uint32_t sym;              /* the tone at the last centre */
  uint32_t nsym;             /* symbols read since the set */
  uint32_t sync_at;          /* nsym at the word that made word sync */
  uint32_t wpos;             /* symbols since the last word, while synced */
  uint32_t synced;
  uint32_t bad;              /* failed words in a row */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t reserved;         /* 0 */
  uint64_t sig, nse;         /* the largest power at the symbols' centres, and 7 / 8 of the mean of the other seven */
  uint64_t ee, el;           /* the smoothed early and late power */
  uint64_t pe, pc, oth;      /* best at the last early point, best and oth at the last centre */
  uint64_t r0, r1, r2;       /* the last 147 bits, the oldest 49 in r0, the first of each in bit 48 */
  int32_t sum[8][2];         /* SI_t, SQ_t at the last completed frame */
  int64_t acc[8][2];         /* I and Q of the open frame, per tone */
} kq_ale_status;
typedef struct kq_ale_event {
  uint32_t word;             /* preamble << 21 | three characters of 7 bits */
  uint32_t flags;            /* bit 0: a half could not be decoded; word holds the data bits as received */
  uint32_t err_a, err_b;     /* bits corrected per half, 4: more than three wrong */
  uint32_t split;            /* places of 49 where the three copies differ */
  uint32_t reserved;         /* 0 */
  uint64_t end_sample;       /* the end of the frame that read the word's last symbol */
  uint64_t sig, nse;         /* at that symbol */
} kq_ale_event;
typedef struct kq_ale_slot {
  uint32_t inc[8];           /* the phase increments of the tones */
  uint32_t tb;               /* the symbol in 1/256 frame */
  uint32_t W;                /* the window in frames */
} kq_ale_slot;

kq_ale_bank *kq_ale_create(const kq_ale_config *cfg);
int kq_ale_destroy(kq_ale_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device, as kq_psk_set */
int kq_ale_set(kq_ale_bank *bank, unsigned slot, const kq_ale_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_ale_remove(kq_ale_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_rtty_process (status may be NULL; nothing is written for an empty slot). */
int kq_ale_process(kq_ale_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_ale_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_ale_pull_counts(kq_ale_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_ale_pull_event(kq_ale_bank *bank, unsigned slot, unsigned index, kq_ale_event *event);
/* Empties every arena (on the handle's stream); the status counters, the register and word sync go on */
int kq_ale_clear_events(kq_ale_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_ale_get_table(const kq_ale_bank *bank, int16_t *dst, size_t cap);
/* inc[8], tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_ale_get_slot(kq_ale_bank *bank, unsigned slot, kq_ale_slot *out);
int kq_ale_sync(kq_ale_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_ale_reset(kq_ale_bank *bank);

/* --- GMDSS digital selective calling (ITU-R M.493) decoder bank -----------------------------------------------------------------
 * Up to 16384 decoder slots, each reading DSC sequences from one audio row, whole messages as events: a receiver bank with
 * a USB channel parked on each of 2187.5, 4207.5, 6312, 8414.5, 12577 and 16804.5 kHz, and a slot on each, keeps the HF /
 * MF watch; VHF channel 70 is read from a flat FM channel resampled to 96 kHz (kq_rsmp_*).  A bank's channels can be decoded
 * in place on its stream after kq_bank_join, and several slots may read one row at different tone pairs.  The reference
 * has no DSC decoder: the algorithm is defined here.  Everything after the quantiser is exact integer arithmetic, so no
 * result depends on how sums are ordered or how the stream is cut into calls.
 * The signal, WRITTEN DOWN FROM MEMORY (no copy of the Recommendation was at hand; ka9q_sdr_amd/itu493.py says the same).
 * 2-FSK, state B is 1 and state Y is 0: 100 baud at 1700 +- 85 Hz on HF / MF, 1200 baud with 1300 Hz (B) and 2100 Hz (Y) on
 * VHF.  Which tone is B turns over with the sideband, so the params name both (mark = B, space = Y) and the sync attempt
 * takes the complement of the register as well.  A symbol is ten bits: seven information bits, the lowest first, then the
 * number of zeros among those seven as three bits, the highest first; 128 of 1024 words are symbols, and any single wrong
 * bit is seen.  Symbol 125 goes out as 1011111001 (the one pattern remembered on its own; tested).  A sequence is a dot
 * pattern (20 or 200 alternating bits) and then the symbol places 0, 1, 2, ..: even places are DX, odd places RX; places 0,
 * 2, .. 10 carry 125; places 1, 3, .. 15 carry 111, 110, .. 104; message symbol i = 0, 1, .. goes out at DX place 12 + 2 i
 * and again at RX place 17 + 2 i, five places (500 ms at 100 baud) later.  Symbols 0 and 1 are both the format specifier;
 * the message ends with an end-of-sequence symbol (117, 122 or 127) and one error-check symbol, the XOR of the information
 * bits of the symbols 1 .. end-of-sequence (one format specifier, not two).  UNVERIFIED against the Recommendation: which
 * audio tone is B on each sideband; the bit order of the count; what the DX places carry while the last RX copies go out
 * (itu493.py repeats the end-of-sequence symbol there; the decoder never reads them); that 117, 122 and 127 appear nowhere
 * inside a message; the layouts of the three messages itu493.py builds; the expansion sequences of M.493-13 and later.
 * Per slot, x[n] is its input row; n counts samples since create or kq_dsc_reset on a grid shared by every slot, and x[n] = 0
 * before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise, table, correlate, window   kq_rtty_*'s, to the letter: q[n], C[j], inc_m = rint(mark 2^32 / Fs) and inc_s
 *              likewise (kq_dsc_get_slot), ph(n) = (n inc) mod 2^32, I and Q per frame and tone below 2^38, reduced a = I >>
 *              12, b = Q >> 12, tb = rint(256 Fs / (B baud)) with 2048 <= tb <= 8192, W = (tb + 128) >> 8 frames, the window
 *              sums SI, SQ over the frames k - W + 1 .. k (zeros before the set), Pm = SIm^2 + SQm^2 and Ps likewise as
 *              uint64, below 2^63.  q = tb >> 2, a quarter bit.  hi = max(Pm, Ps), lo = min(Pm, Ps).
 *   state      frames, ph (0 early, 1 centre, 2 late: the point taken next), t (signed, 1/256 frame, to that point), pe, ee,
 *              el, ec (hi at the last early point; the smoothed early, late and centre), bit, hi and lo (of the last
 *              centre), sig, nse, the register r (64 bits), nbits, synced, bitpos, the counters, and the open message
 *              (kq_dsc_message: inverted, place, nsym, nres, holes, from_rx, run, ecc, eos, hole_mask, sync_sample,
 *              msg[64]).  At the set all zero.
 *   step       one per completed frame k: frames += 1, saturating; t -= 256.  If t >= 128 nothing more happens in this
 *              frame.  Otherwise the frame is a point, taken in turn by ph:
 *                early   pe = hi, t += q, ph = 1.
 *                centre  bit = Pm >= Ps (1 is B), hi and lo are taken, t += q, ph = 2.
 *                late    ph = 0, and with pl = hi the bit is read, in this order:
 *     1 timing    kq_psk_*'s and kq_ale_*'s: ee += (pe - ee) >> 3, el += (pl - el) >> 3 (arithmetic shifts of signed
 *                 differences, here and below); m = max(ee, el); adj = -(tb >> 5) if ee > el and ee - el > (m >> 3), +(tb >> 5)
 *                 if el > ee and el - ee > (m >> 3), else 0; t += tb - 2 q + adj.  At a change of tone the window holds half of
 *                 each and hi dips to a quarter, so the walk settles with the dips half a bit from the centre; through a
 *                 run of equal bits both sides read alike and the clock holds.  Half a bit out the walk has no slope: the
 *                 dips sit on the centre, early and late read alike, and of the starting phases one in twenty or so
 *                 stayed there through a 20-bit dot pattern and lost the message.  So the centre is watched as well: ec +=
 *                 (hi - ec) >> 3, and if adj == 0 and ec + (m >> 3) < min(ee, el) -- the centre reads worse than both
 *                 sides -- t += tb >> 5, one step late, which the walk then takes up.  (|Pm - Ps| in place of hi, which
 *                 falls to nothing at a change of tone, did not cure it in a one-off run on the model.)
 *     2 levels    sig += (hi - sig) >> 4, nse += (lo - nse) >> 4.  open = frames >= warm and sig >= min_p and 16 sig >= snr
 *                 nse, the two products taken exactly (128-bit compare).
 *     3 register  r = (r << 1 | bit) mod 2^64, nbits += 1 (mod 2^32): shifted whether in sync or not.  It holds the last six
 *                 symbol places and four bits, so when the RX copy of a symbol is in bits 9..0 its DX copy, five places
 *                 older, is in bits 59..50.  A ten-bit word w (its first bit sent in bit 9) is a symbol if 7 - popcount(w >>
 *                 3) == (w & 7); its value is the seven bits of w >> 3 reversed.
 *     4 sync      while not synced, and only if open: the attempt on x = r, and if that fails on x = ~r.  s0 = x & 1023, s1 =
 *                 x >> 10 & 1023, s2 = x >> 20 & 1023, s3 = x >> 30 & 1023, the last four places, s0 the latest.  s0 must be a
 *                 symbol of value v, 104 <= v <= 110.  matches = (s2 is the word of v + 1) + (v >= 106 and s1 is the word of
 *                 125) + (v >= 105 and s3 is the word of 125): the places the phasing sequence fixes.  At matches >= acq:
 *                 synced = 1, inverted = (x was ~r), place = 2 (111 - v) + 1, bitpos = 0, the open message emptied (msg all
 *                 0, nsym = nres = holes = from_rx = run = ecc = eos = 0, hole_mask = 0), sync_sample = (k + 1) B, syncs +=
 *                 1.  With acq = 2 there are seven values of s0 and two of three other places exact: noise passes about 7 /
 *                 1024 * 3 / 2^20 = 2e-8 of the attempts, one in 5e7 bits (six days of an open gate at 100 baud).  The step
 *                 ends here.
 *     5 message   while synced (the gate no longer matters: to drop sync on a fade would throw away what the time diversity
 *                 is for): bitpos += 1, and at bitpos == 10: bitpos = 0, place += 1, and if place is odd and >= 17 message
 *                 symbol i = (place - 17) / 2 is resolved.  With x = ~r if inverted, else r: dx = x >> 50 & 1023, rx = x &
 *                 1023.  If dx is a symbol its value d is taken; else if rx is one, its value, and from_rx += 1; else the
 *                 symbol is unresolved.  msg[i] = d, or 0xFF; nsym = i + 1.
 *                   eos == 1     this is the error-check symbol.  flags bit 0 is set if it is unresolved, or holes > 0, or d
 *                                != ecc; an unresolved one counts holes += 1, hole_mask |= 1 << i.  The message is filed,
 *                                rule (a), and synced = 0.
 *                   unresolved   holes += 1, hole_mask |= 1 << i, run += 1.  At run == lose the message ends, rule (c): filed
 *                                with flags bit 2 (and bit 0) if nres >= 8, else aborted += 1, nothing filed; synced = 0.
 *                   resolved     run = 0, nres += 1; if i >= 1, ecc ^= d; if d is 117, 122 or 127, eos = 1.
 *                   then, if still synced and nsym == 64: filed with flags bit 1 (and bit 0), rule (b); synced = 0.
 *   event      sym[64] (msg: the values, 0xFF where unresolved, 0 behind nsym; the last is the error-check symbol where flags
 *              bit 0..2 are clear), nsym, flags (bit 0 the check failed or could not be made, bit 1 truncated at 64
 *              symbols, bit 2 lost, bit 3 the stream was inverted), holes, from_rx, hole_mask, sync_sample, end_sample = (k
 *              + 1) B of the late point that read the last bit, sig and nse there.  events += 1 for each; it goes to the
 *              slot's arena, or dropped += 1 when that holds max_events.  frames, events, dropped, syncs and aborted
 *              saturate at 2^32 - 1.  A single hole can be rebuilt from the error-check symbol on the host
 *              (itu493.repair); the device does not.
 * kq_dsc_remove and kq_dsc_reset discard the open message.  Carried between calls: the open frame's I and Q per tone, the
 * reduced sums of the last 31 frames (W - 1 at the most), the four window sums and all of the state above; so the same
 * stream split differently into calls or blocks gives the same events and status.  kq_dsc_status holds all of it but the
 * past frames.
 * Limits (refused by kq_dsc_create / kq_dsc_set with the reason in kq_last_error, before any HIP call): kq_rtty_*'s --
 * samprate positive and finite; 8 <= B <= 256; warm 0..65535; snr 16..4095; min_p <= 2^55; input_scale > 0; max_slots
 * 1..16384; max_events 1..4096; max_samples 1..2^28; per slot 0 < mark, space < Fs / 2, mark != space, baud positive and
 * finite with 2048 <= tb <= 8192 -- and acq 1..3, lose 1..15.  100 baud fits B = 8..15 at 12 kHz and B = 15..60 at 48 kHz.
 * 1200 baud needs 8 frames of 8 samples in a bit, Fs >= 76.8 kHz: a row from kq_rsmp_* at 96 kHz with B = 8..10.
 * Device memory per slot: 120 max_events of arena, about 800 bytes of state, history and parameters; 2 KiB of table per
 * bank.
 * The default snr of 64 (sig / nse = 4): in the model 240 s of noise alone hold 16 sig / nse between 34 and 74, mean 48.5
 * (the larger of two noise powers is three times the smaller in the mean), and the gate is open at 1282 of 23947 bits; a
 * signal at an Es/N0 of 8 dB holds it between 64 and 174, mean 102, at 10 dB between 91 and 235.  The gate is a squelch on
 * the sync attempt only: noise and a steady tone take no sync and file nothing in 240 s with the gate held open either, by
 * the phasing sequence and the symbol code alone (tests/test_dsc_model.py).  So a gate that opens on noise costs nothing
 * but the attempts, while one that shuts on a weak signal costs messages.
 * NAVTEX / SITOR-B, the other half of the watch (the same modulation and five-place diversity with the CCIR 476 alphabet),
 * is kq_navtex_*, below.  Absent: soft decisions and a bit-wise vote between the copies;
 * AFC; a per-tone threshold under selective fading; the message semantics beyond itu493.py's three builders.  NOTHING HERE
 * HAS MET A SIGNAL OFF THE AIR.  In the model, with white noise, eight individual calls (23 message symbols each behind a
 * 20-bit dot pattern, each in a run of its own) are filed whole with the check good at both (12000, 12) and (39062.5, 32)
 * at an Es/N0 (a tone's power times the bit over N0) of 20, 14 and 12 dB (8 of 8); at 10 dB 7 of 8 at both, and 8 of 8 once
 * itu493.repair has mended the one hole; at 8 dB 2 and 1 of 8 (4 and 4 mended); at 6 dB none.  The fall is steep because a
 * message is whole only if each of its 23 symbols has one of two ten-bit copies without a wrong bit.  At 8 and 6 dB up to
 * three of the eight runs file a message with a symbol that was not sent -- two wrong bits can keep the count right -- and
 * the check catches it.  Measured on the integer model on a CPU (tests/test_dsc_model.py prints the figures); the kernel
 * equals it bit for bit.
 * Calls: as kq_rtty_*.  kq_dsc_create, kq_dsc_set and kq_dsc_remove touch no device. */
typedef struct kq_dsc_bank kq_dsc_bank;
typedef struct kq_dsc_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which no sync is sought while the levels train (64) */
  unsigned snr;              /* least sig / nse for a sync attempt, in sixteenths (64; noise alone gives about 48) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_dsc_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_dsc_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
  unsigned acq;              /* places of the phasing sequence, beside the latest, that must match to take sync, 1..3 (2) */
  unsigned lose;             /* unresolved symbols in a row that end a message, 1..15 (3) */
} kq_dsc_config;
typedef struct kq_dsc_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float mark, space;         /* Hz: state B (1) and state Y (0); 1785 and 1615 are a guess for a USB channel, see above */
  float baud;                /* 100, or 1200 */
} kq_dsc_params;
typedef struct kq_dsc_message {  /* the open (or last) message, as kq_dsc_status carries it */
  uint32_t inverted;         /* sync was taken on the complement of the register */
  uint32_t place;            /* the place of the last whole symbol, while synced */
  uint32_t nsym;             /* message symbols so far */
  uint32_t nres;             /* of them resolved */
  uint32_t holes;            /* and unresolved */
  uint32_t from_rx;          /* resolved by the RX copy */
  uint32_t run;              /* unresolved in a row */
  uint32_t ecc;              /* the XOR so far */
  uint32_t eos;              /* the last symbol was an end of sequence: the next is the error check */
  uint32_t reserved;         /* 0 */
  uint64_t hole_mask;        /* bit i: message symbol i is unresolved */
  uint64_t sync_sample;      /* the end of the frame that took sync */
  uint8_t msg[64];           /* the values, 0xFF where unresolved, 0 behind nsym */
} kq_dsc_message;
typedef struct kq_dsc_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t ph;               /* the point taken next: 0 early, 1 centre, 2 late */
  int32_t t;                 /* 1/256 frame to that point */
  uint32_t bit;              /* at the last centre */
  uint32_t nbits;            /* bits read since the set */
  uint32_t synced;
  uint32_t bitpos;           /* bits of the symbol behind the last whole one, 0..9, while synced */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t syncs;            /* times sync was taken */
  uint32_t aborted;          /* messages that ended by rule (c) with fewer than eight symbols resolved */
  uint32_t reserved;         /* 0 */
  uint64_t sig, nse;         /* the larger and the smaller power at the bits' centres */
  uint64_t ee, el, ec;       /* the smoothed early, late and centre power */
  uint64_t pe, hi, lo;       /* hi at the last early point; hi and lo at the last centre */
  uint64_t r;                /* the last 64 bits, the latest in bit 0 */
  int32_t sum[2][2];         /* SI, SQ of mark and of space at the last completed frame */
  int64_t acc[2][2];         /* I and Q of the open frame, mark and space */
  kq_dsc_message open;
} kq_dsc_status;
typedef struct kq_dsc_event {
  uint8_t sym[64];           /* the message symbols, 0xFF where unresolved, 0 behind nsym */
  uint32_t nsym;
  uint32_t flags;            /* bit 0: check failed or not made; 1: truncated; 2: lost; 3: inverted */
  uint32_t holes;
  uint32_t from_rx;
  uint64_t hole_mask;
  uint64_t sync_sample;
  uint64_t end_sample;       /* the end of the frame that read the message's last bit */
  uint64_t sig, nse;         /* at that bit */
} kq_dsc_event;
typedef struct kq_dsc_slot {
  uint32_t inc_m, inc_s;     /* the phase increments of mark and space */
  uint32_t tb;               /* the bit in 1/256 frame */
  uint32_t W;                /* the window in frames */
} kq_dsc_slot;

kq_dsc_bank *kq_dsc_create(const kq_dsc_config *cfg);
int kq_dsc_destroy(kq_dsc_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device, as kq_rtty_set */
int kq_dsc_set(kq_dsc_bank *bank, unsigned slot, const kq_dsc_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_dsc_remove(kq_dsc_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_rtty_process (status may be NULL; nothing is written for an empty slot). */
int kq_dsc_process(kq_dsc_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride, unsigned block_len,
                   unsigned nblocks, int on_device, kq_dsc_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_dsc_pull_counts(kq_dsc_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_dsc_pull_event(kq_dsc_bank *bank, unsigned slot, unsigned index, kq_dsc_event *event);
/* Empties every arena (on the handle's stream); the status counters, the register and an open message go on */
int kq_dsc_clear_events(kq_dsc_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_dsc_get_table(const kq_dsc_bank *bank, int16_t *dst, size_t cap);
/* inc_m, inc_s, tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_dsc_get_slot(kq_dsc_bank *bank, unsigned slot, kq_dsc_slot *out);
int kq_dsc_sync(kq_dsc_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_dsc_reset(kq_dsc_bank *bank);

/* --- NAVTEX / SITOR-B (CCIR 476, ITU-R M.476 / M.625 collective B mode) decoder bank --------------------------------------
 * Up to 16384 decoder slots, each reading a forward-error-corrected broadcast from one audio row, one event per character:
 * a receiver bank with a USB channel parked on each of 518, 490 and 4209.5 kHz (and on the HF SITOR-B weather and
 * navigational broadcasts), and a slot on each, reads every broadcast at once.  A bank's channels can be decoded in place
 * on its stream after kq_bank_join, and several slots may read one row at different tone pairs.  The host turns the
 * characters into text and ZCZC .. NNNN messages (ka9q_sdr_amd/ccir476.py).  The reference has no NAVTEX decoder: the
 * algorithm is defined here.  Everything after the quantiser is exact integer arithmetic, so no result depends on how sums
 * are ordered or how the stream is cut into calls.
 * The signal, WRITTEN DOWN FROM MEMORY (no copy of the Recommendations was at hand; ccir476.py says the same).  2-FSK, 100
 * baud at 1700 +- 85 Hz, state B is 1 and state Y is 0; B is the higher radio frequency, which on a USB channel with the
 * centre at 1700 Hz makes mark 1785 Hz and space 1615 Hz (kq_dsc_*'s guess, marked as there: the params name both tones,
 * and the sync attempt takes the complement of the register as well).  A character is seven bits of which exactly four
 * are B: the 35 words of that kind are the alphabet (26 letters, CR, LF, LTRS, FIGS, SPACE, BLANK and the three service
 * signals alpha = BBBBYYY = 0x78, beta = BBYYBBY = 0x66, rep = YBBYYBB = 0x33, the first bit sent in bit 6), and any single
 * wrong bit is seen.  The bit stream is a sequence of seven-bit places, alternately DX and RX; character i goes out in DX
 * place 2 i and again in RX place 2 i + 5, 35 bits (350 ms) later.  While phasing -- before a message, between messages,
 * after the last -- the DX places carry rep and the RX places alpha, and so do the places a copy has not reached yet.
 * VERIFIED by tests/test_ccir476.py: that ccir476.py's table uses each of the C(7,4) = 35 words exactly once; and that for
 * the 25 ITA2 combinations with two, three or four marks (the letters other than E and T, and FIGS) bits 2..6 of the word,
 * in sending order, are the ITA2 code in sending order, held against baudot.LETTERS, a table of another origin.  FROM
 * MEMORY ALONE: which of the ten words left over is which of E, T, SPACE, CR, LF, LTRS, BLANK, alpha, beta and rep (the
 * device knows three of them by name: alpha, beta, rep); the international figures case of ccir476.py; the place
 * arithmetic above; which audio tone is B on each sideband.  NOTHING HERE HAS MET A SIGNAL OFF THE AIR.
 * Per slot, x[n] is its input row; n counts samples since create or kq_navtex_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise, table, correlate, window, state (but the register and what is named below), step with its early, centre and
 *   late points, and at the late point
 *     1 timing, 2 levels   kq_dsc_*'s, to the letter (above): q[n], C[j], inc_m, inc_s, tb = rint(256 Fs / (B baud)) within
 *                 2048..8192, W, Pm, Ps, hi, lo, the three-point clock with adj and the centre watch, sig, nse and open.
 *     3 register  r = (r << 1 | bit) mod 2^128, kept as r_hi and r_lo, the latest bit in bit 0 of r_lo; nbits += 1 (mod
 *                 2^32): shifted whether in sync or not.  A seven-bit word w (its first bit sent in bit 6) is a character
 *                 if popcount(w) == 4.
 *     4 sync      while not synced, and only if open: the attempt on x = r, and if that fails on x = ~r (then inverted = 1,
 *                 else 0).  On each x, first the phasing signals, and only if they fail the running traffic.
 *                   phasing   c0 = x & 127, c1 = x >> 7 & 127, c2 = x >> 14 & 127, c3 = x >> 21 & 127, the last four places,
 *                             c0 the latest.  as_rx = (c0 is alpha) + (c1 is rep) + (c2 is alpha) + (c3 is rep); as_dx =
 *                             (c0 is rep) + (c1 is alpha) + (c2 is rep) + (c3 is alpha).  If as_rx >= acq the latest place
 *                             is RX, kind = 1; else if as_dx >= acq it is DX, kind = 0.  Then syncs += 1.  A place equals
 *                             one word at the most, so as_rx + as_dx <= 4 and with acq >= 3 only one of them passes.  The
 *                             phasing stream repeats after 14 bits and after no fewer; its places two apart are equal (c0 =
 *                             c2, c1 = c3).  At an alignment that is off by 1..6 or 8..13 bits the 14 bits read differ
 *                             from both orders of (alpha, rep), so c0 or c1 is wrong, and with it c2 or c3: two matches at
 *                             the most, below either value of acq.  Seven bits off is the other kind of place, not an
 *                             error.  So sync on clean phasing is taken at the right bit and with the right kind or not
 *                             at all; acq = 3 allows one place of four to be damaged.
 *                   traffic   pair j = 0 .. pairs - 1 has its RX copy in bits 14 j + 6 .. 14 j of x and its DX copy in bits
 *                             14 j + 41 .. 14 j + 35 (pairs <= 6: 111 is the highest bit read).  Sync is taken if in every
 *                             one of these pairs the two words are equal, are a character, and are none of alpha, beta
 *                             and rep, and if the pairs do not all hold the same character: a run of one character (a line
 *                             of =, a row of spaces) reads alike with the places' kinds exchanged, and a tracker that
 *                             took the wrong kind would deliver valid-looking wrong text.  Then the latest place is RX,
 *                             kind = 1, and tsyncs += 1.  The characters that served for the sync are not filed: a receiver
 *                             that joins in mid-message reads from the character behind them on.  Noise passes about (35
 *                             / 128 * 1 / 128)^pairs of the attempts, 2e-11 at pairs = 4 (240 s of noise and of a steady
 *                             tone with the gate held open take no sync of either kind in the model).  Traffic at a
 *                             WRONG BIT passes far more often: the copies are 35 bits apart at every bit, so one bit off
 *                             a place six bits of both windows are the same character's still and the seventh agrees by
 *                             chance, about one attempt in four per pair.  Of the late joins in the model (random text,
 *                             every alignment) 2 of 560 took sync at a wrong bit at pairs = 4, none at 6.  Such a sync
 *                             files garbage, much of it unflagged, and chance pairs keep it alive; it ends for certain
 *                             `lose` RX places into the next phasing, which read out of step holds no clean pair.  A
 *                             receiver that must not print garbage sets pairs = 6.
 *                 On either: synced = 1, bitpos = 0, run = 0.  The step ends here.
 *     5 characters  while synced (the gate no longer matters, for kq_dsc_*'s reason): bitpos += 1, and at bitpos == 7: bitpos
 *                 = 0, kind ^= 1, and if kind is now 1 the latest place is an RX place.  With x = ~r if inverted, else r: dx
 *                 = x >> 35 & 127, rx = x & 127.
 *                   run     = 0 if (dx is rep and rx is alpha) or (dx and rx are characters and dx == rx); else run += 1.
 *                   idle    if dx is rep or rx is alpha: idles += 1, nothing is filed.
 *                   else    if dx is a character: code = dx, flags bit 2 if rx is a character and rx != dx; else if rx is
 *                           a character: code = rx, flags bit 1; else code = 0x7F, flags bit 0.  Flags bit 3 if inverted.
 *                           The event is filed.
 *                   then    if run >= lose: synced = 0, losses += 1.
 *                 So sync is held as long as one RX place in `lose` shows a clean pair.  `lose` RX places in a row at which
 *                 one copy alone or neither was good drop it -- a fade of one side alone included, although every
 *                 character of it was read -- and so does a transmission's end, behind which up to `lose` characters of
 *                 garbage (from the RX copy or unresolved in the main) are filed.  This tail is not hidden.
 *   event      code (the word taken, or 0x7F), flags (bit 0 unresolved, bit 1 taken from the RX copy, bit 2 the copies are
 *              two different characters and DX was taken, bit 3 the stream is inverted), dx, rx (the two words as read,
 *              of x), end_sample = (k + 1) B of the late point that read the last bit, sig and nse there.  events += 1 for
 *              each; it goes to the slot's arena, or dropped += 1 when that holds max_events.  frames, events, dropped,
 *              syncs, tsyncs, losses and idles saturate at 2^32 - 1.
 * kq_navtex_remove and kq_navtex_reset discard the sync.  Carried between calls: as kq_dsc_*, and all of the state above; so
 * the same stream split differently into calls or blocks gives the same events and status.  kq_navtex_status holds all of
 * it but the past frames.
 * Limits (refused by kq_navtex_create / kq_navtex_set with the reason in kq_last_error, before any HIP call): kq_dsc_*'s for
 * the fields they share, and acq 3..4, pairs 3..6, lose 1..255.
 * Device memory per slot: 40 max_events of arena, about 700 bytes of state, history and parameters; 2 KiB of table per
 * bank.  At 100 baud an arena of max_events holds max_events / 7.1 seconds of traffic between kq_navtex_clear_events calls.
 * In the model, with white noise, a message of 67 characters behind 20 phasing pairs, four runs (268 characters) at
 * (12000, 12) and at (39062.5, 32): at an Es/N0 (a tone's power times the bit over N0) of 20 and 14 dB every character is
 * read with no flag; at 12 dB none is wrong and 3 and 0 are flagged; at 10 dB 0 and 1 wrong, 8 and 12 flagged; at 8 dB 5 and
 * 10 wrong, 42 and 38 flagged; at 6 dB 58 and 112 wrong.  Measured on the integer model on a CPU
 * (tests/test_navtex_model.py prints the figures, and asserts 20 dB alone); the kernel equals it bit for bit.
 * Absent, beside what kq_dsc_* lacks: the mode-A (ARQ) half of SITOR; a confirmation of the traffic sync (see step 4); a
 * vote that weighs the copies by level; the message store that suppresses a serial number already received (a host's
 * business).
 * Calls: as kq_dsc_*.  kq_navtex_create, kq_navtex_set and kq_navtex_remove touch no device. */
typedef struct kq_navtex_bank kq_navtex_bank;
typedef struct kq_navtex_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which no sync is sought while the levels train (64) */
  unsigned snr;              /* least sig / nse for a sync attempt, in sixteenths (64) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_navtex_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_navtex_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
  unsigned acq;              /* of the last four places, those that must be phasing signals to take sync, 3..4 (4) */
  unsigned pairs;            /* pairs of equal copies that take sync in running traffic, 3..6 (4) */
  unsigned lose;             /* RX places in a row without a clean pair that drop sync, 1..255 (16) */
} kq_navtex_config;
typedef struct kq_navtex_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float mark, space;         /* Hz: state B (1) and state Y (0); 1785 and 1615 are a guess for a USB channel, see above */
  float baud;                /* 100 */
} kq_navtex_params;
typedef struct kq_navtex_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t ph;               /* the point taken next: 0 early, 1 centre, 2 late */
  int32_t t;                 /* 1/256 frame to that point */
  uint32_t bit;              /* at the last centre */
  uint32_t nbits;            /* bits read since the set */
  uint32_t synced;
  uint32_t bitpos;           /* bits of the place behind the last whole one, 0..6, while synced */
  uint32_t kind;             /* of the last whole place: 1 RX, 0 DX */
  uint32_t inverted;         /* sync was taken on the complement of the register */
  uint32_t run;              /* RX places in a row without a clean pair */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t syncs;            /* times sync was taken on the phasing signals */
  uint32_t tsyncs;           /* and on running traffic */
  uint32_t losses;           /* times sync was dropped */
  uint32_t idles;            /* RX places that were phasing */
  uint64_t sig, nse;         /* the larger and the smaller power at the bits' centres */
  uint64_t ee, el, ec;       /* the smoothed early, late and centre power */
  uint64_t pe, hi, lo;       /* hi at the last early point; hi and lo at the last centre */
  uint64_t r_hi, r_lo;       /* the last 128 bits, the latest in bit 0 of r_lo */
  int32_t sum[2][2];         /* SI, SQ of mark and of space at the last completed frame */
  int64_t acc[2][2];         /* I and Q of the open frame, mark and space */
} kq_navtex_status;
typedef struct kq_navtex_event {
  uint32_t code;             /* the seven-bit word taken, the first bit sent in bit 6; 0x7F where unresolved */
  uint32_t flags;            /* bit 0: unresolved; 1: from the RX copy; 2: the copies differ; 3: inverted */
  uint32_t dx, rx;           /* the two words as read */
  uint64_t end_sample;       /* the end of the frame that read the character's last bit */
  uint64_t sig, nse;         /* at that bit */
} kq_navtex_event;
typedef struct kq_navtex_slot {
  uint32_t inc_m, inc_s;     /* the phase increments of mark and space */
  uint32_t tb;               /* the bit in 1/256 frame */
  uint32_t W;                /* the window in frames */
} kq_navtex_slot;

kq_navtex_bank *kq_navtex_create(const kq_navtex_config *cfg);
int kq_navtex_destroy(kq_navtex_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device, as kq_dsc_set */
int kq_navtex_set(kq_navtex_bank *bank, unsigned slot, const kq_navtex_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_navtex_remove(kq_navtex_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_dsc_process (status may be NULL; nothing is written for an empty slot). */
int kq_navtex_process(kq_navtex_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride,
                      unsigned block_len, unsigned nblocks, int on_device, kq_navtex_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_navtex_pull_counts(kq_navtex_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_navtex_pull_event(kq_navtex_bank *bank, unsigned slot, unsigned index, kq_navtex_event *event);
/* Empties every arena (on the handle's stream); the status counters, the register and the sync go on */
int kq_navtex_clear_events(kq_navtex_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_navtex_get_table(const kq_navtex_bank *bank, int16_t *dst, size_t cap);
/* inc_m, inc_s, tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_navtex_get_slot(kq_navtex_bank *bank, unsigned slot, kq_navtex_slot *out);
int kq_navtex_sync(kq_navtex_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_navtex_reset(kq_navtex_bank *bank);

/* --- EAS / SAME (Specific Area Message Encoding; 47 CFR 11.31, NWS Instruction 10-1712) decoder bank -----------------------
 * Up to 16384 decoder slots, each reading the alert headers of one audio row, one event per burst start, per byte of the
 * header and per burst end: a receiver bank or kq_wfm_* that holds thousands of broadcast and weather-radio channels, and a
 * slot on each, says which station relayed which alert and when.  A bank's channels can be decoded in place on its stream
 * after kq_bank_join, and several slots may read one row.  The host votes two of three over the repeats and parses the text
 * (ka9q_sdr_amd/eas.py).  The reference has no SAME decoder: the algorithm is defined here.  Everything after the quantiser
 * is exact integer arithmetic, so no result depends on how sums are ordered or how the stream is cut into calls.
 * The signal, WRITTEN DOWN FROM MEMORY (no copy of the rule or of the Instruction was at hand; eas.py says the same).  AFSK
 * at 520.83 bit/s (a bit is 1.92 ms): mark (1) is 2083.3 Hz, four cycles to a bit, space (0) is 1562.5 Hz, three.  Bytes of
 * eight bits, the least significant bit sent first, bit 7 always 0, no start, stop or parity bit.  A burst is 16 bytes of
 * preamble 0xAB and then the header, ZCZC-ORG-EEE-PSSCCC[-PSSCCC...]+TTTT-JJJHHMM-LLLLLLLL- (1 to 31 location codes, 252
 * bytes at the most), or the end of message, NNNN.  Each is sent three times, one second apart; between the headers and
 * the ends of message stand the attention signal (853 + 960 Hz on broadcast stations, 1050 Hz on weather radio) and the
 * voice message.  There is no checksum: the protection is the threefold repeat, and a receiver votes two of three bit by
 * bit.  FROM MEMORY, all of it: the tone frequencies, the preamble byte and its count, the bit order, the grammar and the
 * names of the fields and event codes in eas.py.  NOTHING HERE HAS MET A SIGNAL OFF THE AIR.
 * Per slot, x[n] is its input row; n counts samples since create or kq_same_reset on a grid shared by every slot, and
 * x[n] = 0 before the slot was set.  Fs = samprate, B = block_len (8..256); frame k is the samples [k B, (k + 1) B).
 *   quantise, table, correlate, window, state (but the register and what is named below), step with its early, centre and
 *   late points, and at the late point
 *     1 timing, 2 levels   kq_dsc_*'s, to the letter (above): q[n], C[j], inc_m, inc_s, tb = rint(256 Fs / (B baud)) within
 *                 2048..8192, W, Pm, Ps, hi, lo, the three-point clock with adj and the centre watch, sig, nse and open.
 *     3 register  r = (r << 1 | bit) mod 2^64, the latest bit in bit 0: shifted whether in sync or not.  The byte
 *                 whose last bit has just arrived is rev8(r & 255), the eight bits turned end for end.
 *     4 sync      while not synced, and only if open.  PH and PE are the 48 bits of the bytes AB AB 'Z' 'C' 'Z' 'C' and AB AB
 *                 'N' 'N' 'N' 'N' in sending order, the first sent highest, each byte turned end for end: 0xD5D55AC25AC2
 *                 and 0xD5D572727272.  dh = popcount((r ^ PH) & (2^48 - 1)), de likewise of PE.
 *                   header    if dh <= sync_errs: synced = 1, bitpos = nbytes = bad_run = plus = dashes = 0, syncs += 1,
 *                             sync_sample = (k + 1) B, and a START event (flags bit 0) with code 'Z' and errs = dh.
 *                   end       else if de <= sync_errs: eoms += 1, sync_sample = (k + 1) B, a START event with code 'N' and
 *                             errs = de; no sync is entered, since nothing follows NNNN.
 *                 Noise passes (1 + 48 + 1128) 2 / 2^48 = 8e-12 of the attempts at sync_errs = 2.  The complement is not
 *                 tried: FM and AM audio do not exchange the tones, and a user on the other sideband exchanges mark and
 *                 space.  The step ends here.
 *     5 text      while synced (the gate no longer matters, for kq_dsc_*'s reason): bitpos += 1, and at bitpos == 8: bitpos
 *                 = 0, b = rev8(r & 255).
 *                   good    0x20 <= b <= 0x7E: an event with code b, flags 0, index = nbytes; bad_run = 0; '+' sets plus =
 *                           1; '-' with plus set counts dashes += 1.
 *                   bad     else: the event is filed all the same with flags bit 1, so that the host's vote has its bits;
 *                           bad_run += 1.
 *                   then    nbytes += 1, and the burst ends at the first of: 1 complete, dashes == 3, the grammar's own
 *                           end (complete += 1); 2 lost, bad_run == lose (lost += 1); 3 length, nbytes == max_len
 *                           (truncated += 1).  An END event (flags bit 2) carries the reason in code and nbytes in
 *                           index, and synced = 0.
 *                 index counts the bytes behind ZCZC, so the first '-' has index 0 and the whole text is "ZCZC" and the
 *                 bytes filed.  A '+' that is read wrong leaves the burst to end by 2 or 3, with garbage behind the
 *                 header's end; the vote over the three bursts mends the text and cuts it at the grammar's end
 *                 (eas.vote, eas.clip).
 *   event      code, flags (bit 0 START, bit 1 BAD, bit 2 END), index, errs (of a START; else 0), end_sample = (k + 1) B of
 *              the late point that read the last bit, sig and nse there.  events += 1 for each; it goes to the slot's
 *              arena, or dropped += 1 when that holds max_events.  frames, events, dropped, syncs, eoms, complete, lost
 *              and truncated saturate at 2^32 - 1.  An alert is at most about 3 * 250 + 9 events.
 * kq_same_remove and kq_same_reset discard the sync.  Carried between calls: as kq_dsc_*, and all of the state above; so the
 * same stream split differently into calls or blocks gives the same events and status.  kq_same_status holds all of it but
 * the past frames.
 * Limits (refused by kq_same_create / kq_same_set with the reason in kq_last_error, before any HIP call): kq_dsc_*'s for the
 * fields they share, and sync_errs 0..4, lose 1..15, max_len 8..248.  A bit wants 8 to 32 frames of at least 8 samples, so
 * Fs >= 33.4 kHz: B = 8..11 at 48 kHz, B = 8..9 at 39 062.5 Hz, B = 8..23 at 96 kHz.  A row at 12 or 24 kHz goes through
 * kq_rsmp_* first, as VHF DSC does.
 * Device memory per slot: 40 max_events of arena, about 700 bytes of state, history and parameters; 2 KiB of table per
 * bank.
 * In the model, with white noise, four alerts of three headers of 42 bytes and three ends of message each, at (48000, 8),
 * (48000, 11) and (39062.5, 8): at an Es/N0 (a tone's power times the bit over N0) of 20, 16 and 14 dB all 12 headers are
 * read with no wrong byte at every geometry; at 12 dB 11, 10 and 12 of them, at 10 dB 4, 4 and 3, at 8 dB none.  The vote of
 * two of three gives the text sent in 4 of 4 alerts down to 12 dB, in 4, 4 and 3 at 10 dB, in 1, 1 and 2 at 8 dB, in none at
 * 6 dB; all 12 ends of message are seen down to 10 dB.  So 14 dB is the lowest level at which every burst came clean.  A
 * sender's clock 100, 1000 and 5000 ppm fast or slow (bits, tones and pauses alike) loses nothing: three of three headers
 * clean and three ends of message at every geometry; 5000 ppm is the largest offset tried, not a limit found.  Measured on
 * the integer model on a CPU (tests/test_same_model.py prints the figures and asserts none of them: the assertions rest
 * on the noise-free cases); the kernel equals the model bit for bit.  60 s of white noise and 60 s of a steady mark tone
 * with the gate forced open (snr 16, min_p 0) file nothing.
 * Absent: the attention signal (two tones or one: kq_tone_*'s business); the vote and the parse on the device (a host's
 * business: eas.py); soft decisions; AFC (the tones are fixed by rule); a confirmation of the sync beyond the 48 bits.
 * Calls: as kq_dsc_*.  kq_same_create, kq_same_set and kq_same_remove touch no device. */
typedef struct kq_same_bank kq_same_bank;
typedef struct kq_same_config {
  int device;
  double samprate;           /* Fs: input samples per second; a double, so that 39 062.5 is exact */
  unsigned block_len;        /* B: samples per frame, 8..256 */
  unsigned warm;             /* frames after the set in which no sync is sought while the levels train (64) */
  unsigned snr;              /* least sig / nse for a sync attempt, in sixteenths (64) */
  uint64_t min_p;            /* least sig (65536) */
  float input_scale;         /* 32767 suits audio of full scale 1 */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 16384) */
  unsigned max_events;       /* arena places per slot between kq_same_clear_events calls */
  size_t max_samples;        /* largest nblocks * block_len of one kq_same_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
  unsigned sync_errs;        /* wrong bits allowed in the 48 that take sync, 0..4 (2) */
  unsigned lose;             /* bad bytes in a row that end a burst, 1..15 (3) */
  unsigned max_len;          /* bytes behind ZCZC at which a burst ends at the latest, 8..248 (248) */
} kq_same_config;
typedef struct kq_same_params {
  unsigned source;           /* input row this slot decodes (a receiver bank's channel index) */
  float mark, space;         /* Hz: 1 and 0; 2083.3333 and 1562.5 */
  float baud;                /* 520.8333 */
} kq_same_params;
typedef struct kq_same_status {
  uint32_t frames;           /* completed since the slot was set */
  uint32_t ph;               /* the point taken next: 0 early, 1 centre, 2 late */
  int32_t t;                 /* 1/256 frame to that point */
  uint32_t bit;              /* at the last centre */
  uint32_t synced;
  uint32_t bitpos;           /* bits of the byte behind the last whole one, 0..7, while synced */
  uint32_t nbytes;           /* bytes of the burst behind ZCZC */
  uint32_t bad_run;          /* bad bytes in a row */
  uint32_t plus;             /* the burst's '+' was seen */
  uint32_t dashes;           /* '-' behind it */
  uint32_t events;           /* filed since the set, those dropped included */
  uint32_t dropped;
  uint32_t syncs;            /* headers begun */
  uint32_t eoms;             /* ends of message seen */
  uint32_t complete;         /* bursts ended by the third dash behind the '+' */
  uint32_t lost;             /* by `lose` bad bytes in a row */
  uint32_t truncated;        /* by max_len */
  uint64_t sync_sample;      /* end_sample of the last START event */
  uint64_t sig, nse;         /* the larger and the smaller power at the bits' centres */
  uint64_t ee, el, ec;       /* the smoothed early, late and centre power */
  uint64_t pe, hi, lo;       /* hi at the last early point; hi and lo at the last centre */
  uint64_t r;                /* the last 64 bits, the latest in bit 0 */
  int32_t sum[2][2];         /* SI, SQ of mark and of space at the last completed frame */
  int64_t acc[2][2];         /* I and Q of the open frame, mark and space */
} kq_same_status;
typedef struct kq_same_event {
  uint32_t code;             /* START: 'Z' or 'N'; a byte as read; END: 1 complete, 2 lost, 3 length */
  uint32_t flags;            /* bit 0: START; 1: BAD (outside 0x20..0x7E); 2: END */
  uint32_t index;            /* of the byte behind ZCZC; END: the bytes read; START: 0 */
  uint32_t errs;             /* START: wrong bits among the 48; else 0 */
  uint64_t end_sample;       /* the end of the frame that read the last bit */
  uint64_t sig, nse;         /* at that bit */
} kq_same_event;
typedef struct kq_same_slot {
  uint32_t inc_m, inc_s;     /* the phase increments of mark and space */
  uint32_t tb;               /* the bit in 1/256 frame */
  uint32_t W;                /* the window in frames */
} kq_same_slot;

kq_same_bank *kq_same_create(const kq_same_config *cfg);
int kq_same_destroy(kq_same_bank *bank);
/* Put a decoder in `slot` (or replace the one there): a cold start at the next call's first sample, its arena empty.
 * Touches no device, as kq_dsc_set */
int kq_same_set(kq_same_bank *bank, unsigned slot, const kq_same_params *params);
/* The slot stops from the next call; its arena stays readable.  Touches no device either */
int kq_same_remove(kq_same_bank *bank, unsigned slot);
/* Input, status and on_device as in kq_dsc_process (status may be NULL; nothing is written for an empty slot). */
int kq_same_process(kq_same_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride,
                    unsigned block_len, unsigned nblocks, int on_device, kq_same_status *status, size_t status_stride);
/* Events in every slot's arena, counts[max_slots], in one copy; synchronous */
int kq_same_pull_counts(kq_same_bank *bank, uint32_t *counts);
/* Copies event `index` of `slot`; returns 0, or -1 */
int kq_same_pull_event(kq_same_bank *bank, unsigned slot, unsigned index, kq_same_event *event);
/* Empties every arena (on the handle's stream); the status counters, the register and the sync go on */
int kq_same_clear_events(kq_same_bank *bank);
/* C (at most cap words); returns 1024 */
int kq_same_get_table(const kq_same_bank *bank, int16_t *dst, size_t cap);
/* inc_m, inc_s, tb and W of `slot`, without a device; -1 when the slot holds no decoder */
int kq_same_get_slot(kq_same_bank *bank, unsigned slot, kq_same_slot *out);
int kq_same_sync(kq_same_bank *bank);
/* Stream index back to 0; every slot restarts cold with its settings at the next call, as if set again */
int kq_same_reset(kq_same_bank *bank);

/* --- rational resampler bank ----------------------------------------------------------------------------------------------
 * Up to 65536 slots, each one row of PCM (mono or stereo) resampled from Fi = in_rate_num / in_rate_den Hz (a receiver
 * bank's samprate and decimate, so 39 062.5 Hz is exact) to Fo = out_rate Hz: kq_afsk_*, RTP PCM and the players are 48 kHz,
 * kq_mon_* wants one rate on a bus, kq_fsk_* 4 to 40 samples per bit, and a receiver channel runs at samprate / decimate.  A
 * receiver bank's audio plane (kq_bank_audio_device_ptr) is resampled on its stream after kq_bank_join(bank); the outputs
 * can go on to kq_afsk_push (session_stride = out_stride, on_device = 1), kq_mon_process (one block of J) and
 * kq_fsk_process without leaving the device.  The reference has no resampler (its front ends are multiples of 48 kHz): the
 * algorithm is defined here.
 *   rates      P / Q = Fo in_rate_den / in_rate_num in lowest terms.
 *   indices    n counts input samples since create or kq_rsmp_reset, j outputs; both are 64-bit and lie on one grid shared
 *              by every slot.  x[n] = 0 before a slot was set.  A KQ_PCM_S16BE word w (network byte order, two's
 *              complement) is SCALE * (short)ntohs(w) as a float product, SCALE = 1.f / SHRT_MAX, as kq_mon_* reads it.
 *   prototype  K = P T taps (T = taps per phase) at rate P Fi, in double: h[m] = sinc(2 cutoff_hz / (P Fi) (m - (K - 1) / 2))
 *              w[m], w = make_kaiser(K, kaiser_beta) (filter.c:337-357), scaled to sum h = P.  g[phi][k] = (float)h[k P + phi]
 *              (kq_rsmp_get_taps).
 *   output j   n_j = floor(j Q / P), phi_j = (j Q) mod P in 64-bit integers; y[j] is the fold acc = fmaf(g[phi_j][k],
 *              x[n_j - k], acc) from 0.0f for k = 0, 1, ..., T - 1 in that order.  This order is part of the contract: it
 *              makes the bits independent of how the stream is cut into calls, blocks and tiles.  A stereo slot filters
 *              its L and R sides separately and writes them interleaved.
 *   delay      the group delay is (K - 1) / (2 P) input samples (kq_rsmp_info::delay_in_samples).
 *   per call   a call that brings the input samples [n0, n0 + S) produces the outputs with n0 <= n_j < n0 + S: J = ceil((n0 +
 *              S) P / Q) - ceil(n0 P / Q) of them, the same for every slot, known without the device, possibly 0.  The last
 *              T - 1 samples of every slot and side are carried across calls, so a call may bring fewer than T, or one.
 *   pcm        the call's own out through scaleclip (audio.c:22-28: >= 1 gives SHRT_MAX, <= -1 SHRT_MIN, else truncation of
 *              SHRT_MAX x; NaN gives 0) in network byte order.
 * NaN and infinity propagate as the float arithmetic gives them: one bad input sample reaches T outputs and no more.
 * Transition band: about 2 Fi sqrt(1 + kaiser_beta^2) / T wide, the window's main lobe (as for kq_wfm_*); a design with no
 * aliasing has cutoff_hz = min(Fi, Fo) / 2 minus half of that.  This is not enforced.
 * Limits (refused with -1 / NULL and the reason in kq_last_error, before any HIP call): 8000 <= Fi, Fo <= 384000; 1/16 <= P / Q
 * <= 16; P <= 4096; 4 <= taps <= 256; P taps <= 2^18; 0 < cutoff_hz < min(Fi, Fo) / 2; kaiser_beta finite and >= 0; max_slots
 * 1..65536; max_samples 1..2^28; channels 1 or 2; kq_rsmp_remove of an empty slot; nblocks block_len > max_samples; nblocks > 1
 * with a block (2 block_len elements where a stereo slot is set) longer than row_stride; out_stride or pcm_stride below c J
 * (c = 2 where a stereo slot is set, else 1); J beyond INT_MAX; an unknown format.
 * Device memory: 16 (taps - 1) + 24 bytes per slot of max_slots (the carried samples of both sides, two copies, and the
 * slot's record) and 4 P taps of coefficients; host-memory calls add their staging buffers.
 * Calls: kq_rsmp_create, kq_rsmp_set and kq_rsmp_remove touch no device; they and kq_rsmp_reset take effect at the first sample
 * of the next kq_rsmp_process, which makes the device half and uploads the slot table when it changed.  A newly set slot
 * starts with zero history on the shared grid, not on a grid of its own.  kq_rsmp_process with device memory is asynchronous
 * on the handle's stream and reads nothing back; with host memory it is synchronous.  A call with no slot set only moves n
 * and j.  One lock per handle. */
typedef struct kq_rsmp_bank kq_rsmp_bank;
typedef struct kq_rsmp_config {
  int device;
  int in_rate_num;           /* Fi = in_rate_num / in_rate_den Hz: a receiver bank's samprate ... */
  int in_rate_den;           /* ... and decimate */
  int out_rate;              /* Fo, Hz */
  unsigned taps;             /* T: taps per phase */
  float cutoff_hz;
  float kaiser_beta;         /* make_kaiser convention */
  unsigned max_slots;        /* slots 0 .. max_slots - 1 (limit 65536) */
  size_t max_samples;        /* largest nblocks * block_len of one kq_rsmp_process call */
  void *stream;              /* hipStream_t, NULL = own stream; kq_bank_stream(bank) puts it beside a receiver bank */
} kq_rsmp_config;
typedef struct kq_rsmp_params {
  unsigned source;           /* input row this slot resamples (a receiver bank's channel index) */
  int channels;              /* 1: mono, 2: interleaved L, R */
} kq_rsmp_params;
typedef struct kq_rsmp_info {
  uint32_t P, Q, taps;
  double delay_in_samples;   /* (P taps - 1) / (2 P) */
  uint64_t next_in, next_out; /* n and j of the next call's first input sample and output */
} kq_rsmp_info;

kq_rsmp_bank *kq_rsmp_create(const kq_rsmp_config *cfg);
int kq_rsmp_destroy(kq_rsmp_bank *bank);
/* Put a resampler in `slot` (or replace the one there): zero history from the next call's first sample */
int kq_rsmp_set(kq_rsmp_bank *bank, unsigned slot, const kq_rsmp_params *params);
/* The slot stops from the next call: its rows are no longer written */
int kq_rsmp_remove(kq_rsmp_bank *bank, unsigned slot);
/* ceil(nsamples P / Q): the J of a call of nsamples never exceeds it (0 and an error for no bank) */
size_t kq_rsmp_max_out(const kq_rsmp_bank *bank, size_t nsamples);
int kq_rsmp_get_info(kq_rsmp_bank *bank, kq_rsmp_info *info);
/* g[phi][k] as used, row by row (at most cap floats); returns P taps */
int kq_rsmp_get_taps(const kq_rsmp_bank *bank, float *dst, size_t cap);
/* Input addressed as in kq_mon_process, in elements of `format` (KQ_PCM_F32 or KQ_PCM_S16BE): block k of row r starts at
 * src[r src_stride + k row_stride]; a mono slot reads block_len values there, a stereo one 2 block_len interleaved L, R.
 * Returns J, or -1.  Slot s writes out[s out_stride + c j + side] for the call's j < J, c = its channels (stride in floats),
 * and pcm[s pcm_stride + c j + side] the same as int16 in network byte order; either may be NULL; nothing is written for an
 * empty slot.  on_device != 0: every pointer is device memory and the call is asynchronous on the handle's stream. */
int kq_rsmp_process(kq_rsmp_bank *bank, const void *src, int format, size_t src_stride, size_t row_stride,
                    unsigned block_len, unsigned nblocks, int on_device, float *out, size_t out_stride, int16_t *pcm,
                    size_t pcm_stride);
int kq_rsmp_sync(kq_rsmp_bank *bank);
/* n and j back to 0; every slot restarts with zero history and its settings */
int kq_rsmp_reset(kq_rsmp_bank *bank);

#ifdef __cplusplus
}
#endif
#endif
