// kq_bank_io.cpp -- samples in, results out: the ring's bookkeeping (note_pushed), kq_bank_push_iq / _push_iq_async /
// _push_zeros / _push_rtp with the run of packet payloads gathered in pinned memory (acc_*), the streaming copies
// (host_io_setup, queue_input_copy, the plane pulls, kq_bank_pull_wait / _host_io_wait), the single-block pulls, the PCM
// stage, RTP out (packetize_block), spectrum capture and the responses' host copies.
// Lock: every entry point takes it through BankScope, kq_bank_rtp_from_planes through LockOnly (and only to look the channel
// up: its packetiser runs without); kq_bank_olen and _last_blocks take none.  kq_bank_pull_wait and _host_io_wait let go of it
// (Unlocked) while they wait for the device.  acc_flush and the file-local functions want it held by the caller.
#include "kq_bank.hpp"

using namespace kq::bank;

namespace {

// What the push entry points refuse, each in the order it always has (kq_bank_push_iq flushes the gathered packets before
// it looks at the format; kq_bank_push_iq_async checks first), and the size of one complex sample of a known format
size_t bytes_per_sample(int format) { return format == KQ_IQ_CF32 ? 8 : format == KQ_IQ_S16 ? 4 : 2; }
int check_format(int format) {
  if (format >= KQ_IQ_CF32 && format <= KQ_IQ_S8) return 0;
  kq_internal_set_error("unknown I/Q format %d", format);
  return -1;
}
// samples in the ring, the M - 1 of history included: where the next push lands
size_t ring_used(const kq_bank *b) { return (size_t)(b->g.M - 1) + b->pending; }
// `counts`: the refusal gives them (kq_bank_push_zeros' does not)
int check_ring_room(const kq_bank *b, size_t nsamples, bool counts = true) {
  if (ring_used(b) + nsamples <= b->ring_cap) return 0;
  if (counts)
    kq_internal_set_error("ring overflow: %zu pending + %zu pushed > %zu", b->pending, nsamples, b->ring_cap - (b->g.M - 1));
  else
    kq_internal_set_error("ring overflow");
  return -1;
}

// block completion bookkeeping for the IF-power rule (radio.c:140-146 against radio.c:94-98)
void note_pushed(kq_bank *b, size_t nsamples, unsigned char zero) {
  size_t fill = b->pending % b->g.L, left = nsamples;
  while (left) {
    size_t const take = std::min(left, (size_t)b->g.L - fill);
    fill += take;
    left -= take;
    if (fill == (size_t)b->g.L) {
      b->zero_tail.push_back(zero);
      fill = 0;
    }
  }
  b->pending += nsamples;
}

int host_io_setup(kq_bank *b) {
  if (b->copy_in) return 0;
  // Streams share a handful of hardware queues, handed out in creation order, and a queue runs in order: the two copy
  // streams can land on one queue.  Then an input copy queued BEHIND an output copy waits with it for that call's
  // demodulators, and every step runs input copy, kernels and output copy one after the other (rocprofv3 timeline,
  // tools/hostio_trace.sh) -- hence the call order the header asks for: push batch k+1 before pulling the planes of
  // batch k.  (Streams of different priority come from different queue pools, but with a high-priority output stream
  // the filter kernel itself ran 40 % slower for the whole step, measured.)
  if (b->new_stream(&b->copy_in) || b->new_stream(&b->copy_out)) return -1;
  for (int k = 0; k < 2; k++)
    if (b->new_event(&b->in_ready[k], hipEventDisableTiming) || b->new_event(&b->in_free[k], hipEventDisableTiming)) return -1;
  if (b->new_event(&b->out_ready, hipEventDisableTiming)) return -1;
  for (hipEvent_t &e : b->pull_done)
    if (b->new_event(&e, hipEventDisableTiming)) return -1;
  return 0;
}

// `nsamples` samples of `format` in pinned host memory -> staging buffer (copy stream) -> conversion kernel (bank's stream)
// into the ring at sample offset `ring_off`.  Nothing waits on the host but the reuse of a staging buffer two copies later.
int queue_input_copy(kq_bank *b, const void *iq, size_t nsamples, int format, size_t ring_off) {
  if (host_io_setup(b)) return -1;
  size_t const bps = bytes_per_sample(format);
  int const k = b->in_next;
  b->in_next ^= 1;
  if (b->in_stage_cap[k] < nsamples * bps) {
    KQ_TRY(hipStreamSynchronize(b->copy_in));  // (grow waits for the main stream: the conversion kernels)
    if (b->grow(&b->in_stage[k], &b->in_stage_cap[k], nsamples * bps)) return -1;
  }
  // The header's promise -- `iq` may be reused once two more pushes have been queued -- is kept here: the push two
  // back used this staging index, and its host-to-device copy must have READ the caller's buffer before this call
  // returns (a device-side wait alone would let the host run ahead of the copy engine).  Normally long done.
  if (b->in_used[k]) KQ_TRY(hipEventSynchronize(b->in_ready[k]));
  b->in_used[k] = true;
  KQ_TRY(hipStreamWaitEvent(b->copy_in, b->in_free[k], 0));  // the conversion kernel that last read this buffer
  KQ_TRY(hipMemcpyAsync(b->in_stage[k], iq, nsamples * bps, hipMemcpyHostToDevice, b->copy_in));
  KQ_TRY(hipEventRecord(b->in_ready[k], b->copy_in));
  KQ_TRY(hipStreamWaitEvent(b->stream, b->in_ready[k], 0));
  {
    Scope t(b, 2, b->stream);
    kq::launch_ingest(b->stream, b->in_stage[k], format, b->ring[b->cur] + ring_off, nsamples, b->cfg.gain_factor);
  }
  KQ_TRY(hipEventRecord(b->in_free[k], b->stream));
  return 0;
}

// one packet's payload (host memory, any alignment) joins the run; the bookkeeping of the ring moves at once
int acc_append(kq_bank *b, const void *src, size_t nsamples, int format) {
  if (nsamples == 0) return 0;
  size_t const bps = bytes_per_sample(format);
  if (!b->acc_pin[0]) {
    b->acc_cap = b->ring_cap * 8;  // the whole ring in the widest format
    for (int k = 0; k < 2; k++) {
      if (b->alloc_pinned(&b->acc_pin[k], b->acc_cap) || b->new_event(&b->acc_read[k], hipEventDisableTiming)) return -1;
    }
  }
  if (b->acc_n && (format != b->acc_fmt || (b->acc_n + nsamples) * bps > b->acc_cap) && acc_flush(b)) return -1;
  if (b->acc_n == 0) {
    b->acc_fmt = format;
    b->acc_ring_off = ring_used(b);
  }
  memcpy(b->acc_pin[b->acc_cur] + b->acc_n * bps, src, nsamples * bps);
  b->acc_n += nsamples;
  note_pushed(b, nsamples, 0);
  return 0;
}

// the copy stream gets behind the last call's demodulators: their own marker when they ran on their own stream, else one
// on the main stream
int pull_prologue(kq_bank *b) {
  if (!b || b->calls == 0) {
    kq_internal_set_error("nothing processed yet");
    return -1;
  }
  if (host_io_setup(b)) return -1;
  int const last = (int)((b->calls - 1) & 1);
  if (b->demod_overlapped[last]) {
    KQ_TRY(hipStreamWaitEvent(b->copy_out, b->ev_demod_done[last], 0));
  } else {
    KQ_TRY(hipEventRecord(b->out_ready, b->stream));
    KQ_TRY(hipStreamWaitEvent(b->copy_out, b->out_ready, 0));
  }
  b->pulled_since_call = true;
  return 0;
}
int pull_epilogue(kq_bank *b) {
  KQ_TRY(hipEventRecord(b->pull_done[b->pulls % kq_bank::kPullRing], b->copy_out));
  b->pulls++;
  b->out_pending = true;
  return 0;
}

// The reference's real output format (audio.c:22-28, 45-50, 95-100): clipped int16 in network byte order, half the bytes
// of the float plane.  The conversion runs inside the copy kernel (the same arithmetic as k_pcm, the stage behind
// kq_bank_enable_pcm, which this call does not need).
int pull_pcm_planes(kq_bank *b, int16_t *pcm, uint32_t *silent_mask, void *status, bool compact) {
  BankScope dev_scope_(b);
  if (!pcm) {
    kq_internal_set_error("NULL pcm plane");
    return -1;
  }
  bool const aligned = (reinterpret_cast<uintptr_t>(pcm) & 15) == 0 && (reinterpret_cast<uintptr_t>(status) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(silent_mask) & 3) == 0;
  if (b && (b->g.olen % 8 != 0 || !aligned || 2 * (size_t)b->g.olen > 32 * 480)) {
    kq_internal_set_error("kq_bank_pull_pcm_planes_async: olen must be a multiple of 8 and at most 7680, the planes 16-byte aligned");
    return -1;
  }
  if (pull_prologue(b)) return -1;
  size_t const n = b->chans.size() * (size_t)b->g.max_blocks;
  size_t const sbytes = n * sizeof(kq_chan_status), s16 = sbytes & ~(size_t)15;
  kq::launch_copy_pcm_to_host(b->copy_out, b->pl.audio, pcm, silent_mask, 2 * b->g.olen, b->pl.status, status, n,
                              compact && status ? b->chd.mode : nullptr, b->g.max_blocks);
  LAUNCH_CHECK("PCM plane copy");
  if (status && !compact && sbytes > s16)
    KQ_TRY(hipMemcpyAsync((char *)status + s16, (const char *)b->pl.status + s16, sbytes - s16, hipMemcpyDeviceToHost, b->copy_out));
  return pull_epilogue(b);
}

// send_mono_output / send_stereo_output (audio.c:32-132) on the words of one channel-block: 480-word chunks, all-zero
// chunks skipped while the timestamp still advances, marker bit on the first packet after silence, sequence numbers on
// sent packets only.  `w`: nwords int16 in network byte order.  Packets back to back as [2-byte LE length][bytes].
int packetize_block(kq_out_rtp_state &o, const unsigned char *w, size_t nwords, bool stereo, unsigned char *dst, size_t cap,
                    size_t *used) {
  size_t pos = 0, left = nwords;
  int packets = 0;
  while (left > 0) {
    size_t const chunk = std::min<size_t>(480, left);  // PCM_BUFSIZE words, audio.c:19,44,94
    bool not_silent = false;
    for (size_t i = 0; i < 2 * chunk; i++) not_silent |= w[i] != 0;
    uint32_t const ts = o.timestamp;
    o.timestamp += (uint32_t)(stereo ? chunk / 2 : chunk);  // audio.c:52-53,103-104: advances even when nothing is sent
    if (not_silent) {
      o.packets++;
      o.bytes += (int64_t)(2 * chunk);
      int marker = 0;
      if (o.silent) {  // audio.c:57-61,109-113
        o.silent = 0;
        marker = 1;
      }
      uint16_t const seq = o.seq++;
      size_t const len = 12 + 2 * chunk;
      if (pos + 2 + len > cap) {
        kq_internal_set_error("packet buffer too small");
        return -1;
      }
      unsigned char *dp = dst + pos;
      dp[0] = (unsigned char)len;
      dp[1] = (unsigned char)(len >> 8);
      dp += 2;
      dp[0] = 2 << 6;  // RTP version 2; no padding, extension or CSRCs (multicast.c:285)
      dp[1] = (unsigned char)((marker << 7) | (stereo ? 10 : 11));
      dp[2] = (unsigned char)(seq >> 8);
      dp[3] = (unsigned char)seq;
      for (int k = 0; k < 4; k++) dp[4 + k] = (unsigned char)(ts >> (24 - 8 * k));
      for (int k = 0; k < 4; k++) dp[8 + k] = (unsigned char)(o.ssrc >> (24 - 8 * k));
      memcpy(dp + 12, w, 2 * chunk);
      pos += 2 + len;
      packets++;
    } else {
      o.silent = 1;
    }
    w += 2 * chunk;
    left -= chunk;
  }
  if (used) *used = pos;
  return packets;
}

}  // namespace

// the gathered run of packet payloads goes out (see acc_pin)
int kq::bank::acc_flush(kq_bank *b) {
  if (b->acc_n == 0) return 0;
  int const j = b->acc_cur;
  if (queue_input_copy(b, b->acc_pin[j], b->acc_n, b->acc_fmt, b->acc_ring_off)) return -1;
  KQ_TRY(hipEventRecord(b->acc_read[j], b->copy_in));
  b->acc_read_set[j] = true;
  b->acc_cur ^= 1;
  b->acc_n = 0;
  // the buffer gathered into next was handed to the copy engine two flushes ago
  if (b->acc_read_set[b->acc_cur]) KQ_TRY(hipEventSynchronize(b->acc_read[b->acc_cur]));
  return 0;
}

extern "C" {

int kq_bank_push_iq(kq_bank *b, const void *iq, size_t nsamples, int format, int is_device) {
  BankScope dev_scope_(b);
  if (!b || (!iq && nsamples)) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  if (acc_flush(b)) return -1;  // packet payloads gathered by kq_bank_push_rtp go first
  if (check_format(format) || check_ring_room(b, nsamples)) return -1;
  size_t const used = ring_used(b), bps = bytes_per_sample(format);
  const void *src = iq;
  if (!is_device) {
    if (b->grow(&b->stage_dev, &b->stage_cap, nsamples * bps)) return -1;
    KQ_TRY(hipMemcpyAsync(b->stage_dev, iq, nsamples * bps, hipMemcpyHostToDevice, b->stream));
    src = b->stage_dev;
  }
  {
    Scope t(b, 2, b->stream);
    kq::launch_ingest(b->stream, src, format, b->ring[b->cur] + used, nsamples, b->cfg.gain_factor);
  }
  if (!is_device) KQ_TRY(hipStreamSynchronize(b->stream));  // the caller may reuse iq
  note_pushed(b, nsamples, 0);
  return 0;
}

int kq_bank_push_iq_async(kq_bank *b, const void *iq, size_t nsamples, int format) {
  BankScope dev_scope_(b);
  if (!b || (!iq && nsamples)) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  if (check_format(format) || check_ring_room(b, nsamples)) return -1;
  size_t const used = ring_used(b);
  if (nsamples == 0) return 0;
  if (acc_flush(b)) return -1;
  if (queue_input_copy(b, iq, nsamples, format, used)) return -1;
  note_pushed(b, nsamples, 0);
  return 0;
}

int kq_bank_pull_planes_async(kq_bank *b, float *audio, kq_chan_status *status) {
  BankScope dev_scope_(b);
  if (pull_prologue(b)) return -1;
  size_t const n = b->chans.size() * (size_t)b->g.max_blocks;
  // of every channel-block's 2 * olen floats only the status.nout that hold samples travel (mono: half): the kernel
  // moves 16 bytes per lane, so olen must be a multiple of 4 for it -- other geometries take the plain copy
  size_t const sbytes = n * sizeof(kq_chan_status), s16 = sbytes & ~(size_t)15;
  // (memory from kq_host_alloc is page aligned; anything less than 16 bytes takes the plain copies)
  bool const aligned = (reinterpret_cast<uintptr_t>(audio) & 15) == 0 && (reinterpret_cast<uintptr_t>(status) & 15) == 0;
  bool const rows_ok = b->g.olen % 4 == 0 && aligned;
  if (!aligned) {
    if (audio)
      KQ_TRY(hipMemcpyAsync(audio, b->pl.audio, n * 2 * (size_t)b->g.olen * sizeof(float), hipMemcpyDeviceToHost, b->copy_out));
    if (status) KQ_TRY(hipMemcpyAsync(status, b->pl.status, sbytes, hipMemcpyDeviceToHost, b->copy_out));
    return pull_epilogue(b);
  }
  kq::launch_copy_to_host(b->copy_out, b->pl.audio, rows_ok ? audio : nullptr, 2 * b->g.olen, b->pl.status, status, n);
  LAUNCH_CHECK("plane copy");
  if (audio && !rows_ok)
    KQ_TRY(hipMemcpyAsync(audio, b->pl.audio, n * 2 * (size_t)b->g.olen * sizeof(float), hipMemcpyDeviceToHost, b->copy_out));
  if (status && sbytes > s16)
    KQ_TRY(hipMemcpyAsync((char *)status + s16, (const char *)b->pl.status + s16, sbytes - s16, hipMemcpyDeviceToHost, b->copy_out));
  return pull_epilogue(b);
}

int kq_bank_pull_pcm_planes_async(kq_bank *b, int16_t *pcm, uint32_t *silent_mask, kq_chan_status *status) {
  return pull_pcm_planes(b, pcm, silent_mask, status, false);
}
// ... with the 24 bytes of every status record a receiver reads per block (include/ka9q_hip.h kq_chan_status_compact)
int kq_bank_pull_pcm_planes_compact_async(kq_bank *b, int16_t *pcm, uint32_t *silent_mask, kq_chan_status_compact *status) {
  return pull_pcm_planes(b, pcm, silent_mask, status, true);
}

int kq_bank_pull_wait(kq_bank *b, unsigned lag) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  if (lag >= (unsigned)kq_bank::kPullRing) {
    kq_internal_set_error("kq_bank_pull_wait: lag %u, at most %d deliveries are remembered", lag, kq_bank::kPullRing - 1);
    return -1;
  }
  if (b->pulls <= lag) return 0;  // nothing that far back was ever queued
  hipEvent_t const ev = b->pull_done[(b->pulls - 1 - lag) % kq_bank::kPullRing];
  {
    Unlocked u(dev_scope_);  // (the ring holds kPullRing deliveries: the event is not recorded again before this one is long over)
    KQ_TRY(hipEventSynchronize(ev));
  }
  return report_lost_sibling(b);
}

int kq_bank_host_io_wait(kq_bank *b) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  hipStream_t const cin = b->copy_in, cout = b->copy_out;  // (read under the lock: host_io_setup may be creating them)
  {
    Unlocked u(dev_scope_);
    if (cin) KQ_TRY(hipStreamSynchronize(cin));
    if (cout) KQ_TRY(hipStreamSynchronize(cout));
  }
  return report_lost_sibling(b);  // the planes just landed come from kernels that have finished
}

int kq_bank_push_zeros(kq_bank *b, size_t nsamples) {
  BankScope dev_scope_(b);
  if (!b) {
    kq_internal_set_error("NULL bank");
    return -1;
  }
  if (check_ring_room(b, nsamples, false)) return -1;
  size_t const used = ring_used(b);
  if (acc_flush(b)) return -1;
  KQ_TRY(hipMemsetAsync(b->ring[b->cur] + used, 0, nsamples * sizeof(float2), b->stream));
  note_pushed(b, nsamples, 1);  // (blocks completed inside radio.c:88-99)
  return 0;
}

int kq_bank_push_rtp(kq_bank *b, const void *datagram, size_t size) {
  BankScope dev_scope_(b);
  if (!b || !datagram) {
    kq_internal_set_error("NULL argument");
    return -1;
  }
  const unsigned char *p = static_cast<const unsigned char *>(datagram);
  auto be16 = [](const unsigned char *q) { return (unsigned)((q[0] << 8) | q[1]); };
  auto be32 = [](const unsigned char *q) { return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3]; };
  if (size < 12) return 0;  // RTP_MIN_SIZE, main.c:315-316
  // RTP header (multicast.c:242-277)
  bool const pad = (p[0] >> 5) & 1, ext = (p[0] >> 4) & 1;
  unsigned const cc = p[0] & 0xf;
  unsigned const type = p[1] & 0x7f;
  uint16_t const seq = (uint16_t)be16(p + 2);
  uint32_t const ts = be32(p + 4), ssrc = be32(p + 8);
  size_t hdr = 12 + 4 * (size_t)cc;
  if (ext) {
    if (hdr + 4 > size) return 0;
    hdr += 4 + 4 + be16(p + hdr + 2);  // type, length, and the reference's "4 + length" bytes
  }
  if (hdr > size) return 0;
  size_t len = size - hdr;
  if (pad && len > 0) {  // main.c:324-328
    unsigned const npad = p[size - 1];
    if (npad > len) return 0;
    len -= npad;
  }
  if (type != 97 && type != 98) return 0;  // IQ_PT / IQ_PT8, main.c:329-330
  if (len < 24) return 0;
  hdr += 24;  // obsolete status block, main.c:338-341
  len -= 24;
  int const sampcount = (int)(type == 97 ? len / 4 : len / 2);  // radio.c:64-72

  // proc_samples + rtp_process (radio.c:73-104, multicast.c:305-340)
  kq_rtp_counters &r = b->rtp;
  if (!b->rtp_init || ssrc != r.ssrc) {
    r.samples = 0;  // radio.c:73-77 (a fresh state has ssrc 0, so the first packet lands here as well)
    r.ssrc = ssrc;
    r.packets = 0;
    r.next_seq = seq;
    r.next_timestamp = ts;
    r.dupes = 0;
    r.drops = 0;
    b->rtp_init = true;
    b->rtp_retry = false;
  }
  // A datagram handed in again after -2 is the same packet, not a new one: it is counted once.
  bool const retry = b->rtp_retry && seq == b->rtp_retry_seq && ts == b->rtp_retry_ts;
  b->rtp_retry = false;
  short const seq_step = (short)(seq - r.next_seq);
  if (seq_step < 0) {
    r.packets++;
    r.dupes++;
    return 0;
  }
  int const time_step = (int)(ts - r.next_timestamp);
  if (time_step < 0 || time_step > 192000) {  // old samples (multicast.c:334-336) / a jump too far to fill (radio.c:79-82)
    if (!retry) r.packets++;
    r.drops += seq_step;
    r.next_seq = (uint16_t)(seq + 1);
    if (time_step >= 0) r.next_timestamp = ts + (uint32_t)sampcount;
    return 0;
  }
  // Room.  The ring takes max_blocks * L samples plus L - 1 of slack, so that a partly filled block never stands in the
  // way of a packet that fits the ring as such.  What does not fit now:
  //  * whole blocks are waiting (pending >= L): nothing moves, -2 -- kq_bank_process frees them, then the same datagram
  //    fits or falls under the next case;
  //  * no whole block is waiting, so the zero fill of the gap (radio.c:83-100) is itself larger than the ring: as many
  //    zeros as fit go in now and the timestamp moves past them, -2 -- every retry after a kq_bank_process brings the
  //    gap a ring closer to its end, with the oscillators running through it sample by sample as in the reference;
  //  * the gap is filled and the payload alone is larger than the ring (max_blocks * L below one packet): -1, the
  //    sequence number moves on, the timestamp does not, so the next packet fills these samples with zeros.
  size_t const room = b->ring_cap - ring_used(b);
  size_t const payload = (size_t)(sampcount > 0 ? sampcount : 0);
  if ((size_t)time_step + payload > room) {
    if (b->pending >= (size_t)b->g.L) {  // nothing has moved: not the sequence number, not the timestamp, not a counter
      b->rtp_retry = retry;
      kq_internal_set_error("ring full: %zu samples pending, the packet brings %zu (zero fill %d): run kq_bank_process, then push it again",
              b->pending, (size_t)time_step + payload, time_step);
      return -2;
    }
    if (time_step > 0) {
      size_t const z = std::min((size_t)time_step, room);
      if (kq_bank_push_zeros(b, z)) return -1;
      if (!retry) r.packets++;
      r.samples += (int)z;
      r.next_timestamp += (uint32_t)z;
      r.drops += seq_step;
      r.next_seq = seq;  // the retry is in sequence
      b->rtp_retry = true;
      b->rtp_retry_seq = seq;
      b->rtp_retry_ts = ts;
      kq_internal_set_error("the gap's zero fill is larger than the ring: %zu of %d samples in, run kq_bank_process, then push it again", z,
              time_step);
      return -2;
    }
    if (!retry) r.packets++;
    r.drops += seq_step;
    r.next_seq = (uint16_t)(seq + 1);
    kq_internal_set_error("a packet of %zu samples does not fit a ring of %zu: raise max_blocks", payload, b->ring_cap - (size_t)(b->g.M - 1));
    return -1;
  }
  if (!retry) r.packets++;
  r.drops += seq_step;
  r.next_seq = (uint16_t)(seq + 1);
  r.next_timestamp = ts + (uint32_t)sampcount;
  if (time_step > 0) {
    if (kq_bank_push_zeros(b, (size_t)time_step)) return -1;  // radio.c:83-100
    r.samples += time_step;
  }
  r.samples += sampcount;
  // the payload joins the run gathered in pinned memory: one asynchronous copy and one conversion per run, not per packet
  if (sampcount > 0 && acc_append(b, p + hdr, (size_t)sampcount, type == 97 ? KQ_IQ_S16 : KQ_IQ_S8)) return -1;
  return time_step + sampcount;
}

int kq_bank_rtp_counters(const kq_bank *b, kq_rtp_counters *out) {
  BankScope dev_scope_(b);
  if (!b || !out) return -1;
  *out = b->rtp;
  return 0;
}

unsigned kq_bank_olen(const kq_bank *b) { return b ? (unsigned)b->g.olen : 0; }
unsigned kq_bank_last_blocks(const kq_bank *b) { return b ? b->last_blocks : 0; }

int kq_bank_pull_status(kq_bank *b, int ch, unsigned blk, kq_chan_status *st) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !st || blk >= b->last_blocks) {
    kq_internal_set_error("bad channel/block");
    return -1;
  }
  if (sync_all(b)) return -1;
  KQ_TRY(hipMemcpy(st, b->pl.status + (size_t)ch * b->g.max_blocks + blk, sizeof(*st), hipMemcpyDeviceToHost));
  return 0;
}

int kq_bank_pull_audio(kq_bank *b, int ch, unsigned blk, float *dst, size_t cap, size_t *n) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || blk >= b->last_blocks) {
    kq_internal_set_error("bad channel/block");
    return -1;
  }
  kq_chan_status st;
  if (kq_bank_pull_status(b, ch, blk, &st)) return -1;
  if ((size_t)st.nout > cap) {
    kq_internal_set_error("audio buffer too small: %d > %zu", st.nout, cap);
    return -1;
  }
  KQ_TRY(hipMemcpy(dst, b->pl.audio + ((size_t)ch * b->g.max_blocks + blk) * 2 * (size_t)b->g.olen, st.nout * sizeof(float),
                    hipMemcpyDeviceToHost));
  if (n) *n = (size_t)st.nout;
  return 0;
}

int kq_bank_enable_pcm(kq_bank *b, int on) {
  BankScope dev_scope_(b);
  if (!b) return -1;
  if (on && 2 * (size_t)b->g.olen > 32 * 480) {
    // the silent-packet mask of kq_bank_pull_pcm is 32 bits: one per 480-word packet of a block
    kq_internal_set_error("PCM stage: %d output samples per block make more than 32 packets", b->g.olen);
    return -1;
  }
  if (on && !b->pcm) {
    size_t const CB = (size_t)b->cfg.max_channels * b->cfg.max_blocks;
    if (alloc_cleared(b, &b->pcm, CB * 2 * (size_t)b->g.olen) || alloc_cleared(b, &b->pcm_mask, CB)) return -1;
  }
  b->pcm_on = on != 0;
  return 0;
}

int kq_bank_pull_pcm(kq_bank *b, int ch, unsigned blk, int16_t *dst, size_t cap, size_t *nwords, uint32_t *silent_mask) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || blk >= b->last_blocks || !b->pcm_on) {
    kq_internal_set_error("bad channel/block, or PCM stage not enabled");
    return -1;
  }
  kq_chan_status st;
  if (kq_bank_pull_status(b, ch, blk, &st)) return -1;
  if ((size_t)st.nout > cap) {
    kq_internal_set_error("PCM buffer too small");
    return -1;
  }
  size_t const cb = (size_t)ch * b->g.max_blocks + blk;
  KQ_TRY(hipMemcpy(dst, b->pcm + cb * 2 * (size_t)b->g.olen, st.nout * sizeof(int16_t), hipMemcpyDeviceToHost));
  uint32_t m = 0;
  KQ_TRY(hipMemcpy(&m, b->pcm_mask + cb, sizeof(m), hipMemcpyDeviceToHost));
  if (nwords) *nwords = (size_t)st.nout;
  if (silent_mask) *silent_mask = m;
  return 0;
}

int kq_bank_set_output_ssrc(kq_bank *b, int ch, uint32_t ssrc) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch)) {
    kq_internal_set_error("bad channel");
    return -1;
  }
  b->chans[ch].out_rtp.ssrc = ssrc;
  return 0;
}

int kq_bank_output_rtp_state(const kq_bank *b, int ch, kq_out_rtp_state *out) {
  BankScope dev_scope_(b);
  if (!out || !valid_ch(b, ch)) return -1;
  *out = b->chans[ch].out_rtp;
  return 0;
}

int kq_bank_pull_rtp_audio(kq_bank *b, int ch, unsigned blk, unsigned char *dst, size_t cap, size_t *used) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst) {
    kq_internal_set_error("bad channel or NULL buffer");
    return -1;
  }
  std::vector<int16_t> words(2 * (size_t)b->g.olen);
  size_t nwords = 0;
  if (kq_bank_pull_pcm(b, ch, blk, words.data(), words.size(), &nwords, nullptr)) return -1;
  bool const stereo = nwords == 2 * (size_t)b->g.olen;  // what the demodulator passed to send_stereo_output
  return packetize_block(b->chans[ch].out_rtp, reinterpret_cast<const unsigned char *>(words.data()), nwords, stereo, dst, cap, used);
}

// The same datagrams from planes the host already holds (kq_bank_pull_pcm_planes_async): no device access, no wait.
int kq_bank_rtp_from_planes(kq_bank *b, int ch, unsigned blk, const int16_t *pcm_plane, const kq_chan_status *status_plane,
                            unsigned char *dst, size_t cap, size_t *used) {
  if (!b) {
    kq_internal_set_error("NULL bank");
    return -1;
  }
  // Host work only, and meant to be spread over the host's threads by channel range: the bank's lock is held just long
  // enough to check the channel and take the address of its RTP state (b->chans is reserved for max_channels at create:
  // its elements never move).  One thread per channel at a time -- the caller's partition -- owns that state; a channel
  // removed or restarted while its packetiser runs is the caller's race, as two threads in audio.c:82 would be.
  kq_out_rtp_state *o = nullptr;
  int olen = 0, max_blocks = 0;
  {
    LockOnly lk(b);
    if (!valid_ch(b, ch) || !dst || !pcm_plane || !status_plane || blk >= (unsigned)b->g.max_blocks) {
      kq_internal_set_error("bad channel / block or NULL plane");
      return -1;
    }
    o = &b->chans[ch].out_rtp;
    olen = b->g.olen;
    max_blocks = b->g.max_blocks;
  }
  size_t const cb = (size_t)ch * max_blocks + blk;
  int const nout = status_plane[cb].nout;
  if (nout < 0 || nout > 2 * olen) {
    kq_internal_set_error("status plane: nout %d out of range", nout);
    return -1;
  }
  return packetize_block(*o, reinterpret_cast<const unsigned char *>(pcm_plane + cb * 2 * (size_t)olen), (size_t)nout,
                         nout == 2 * olen, dst, cap, used);
}

int kq_bank_pull_filter_output(kq_bank *b, int ch, unsigned blk, float *dst, size_t cap) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || blk >= b->last_blocks || cap < (size_t)b->g.olen) {
    kq_internal_set_error("bad channel/block/capacity");
    return -1;
  }
  if (sync_all(b)) return -1;
  KQ_TRY(hipMemcpy(dst, b->pl.filt + ((size_t)ch * b->g.max_blocks + blk) * b->g.olen, b->g.olen * sizeof(float2),
                    hipMemcpyDeviceToHost));
  return 0;
}

int kq_bank_pull_pl_samples(kq_bank *b, int ch, unsigned blk, float *dst, size_t cap, size_t *n) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || blk >= b->last_blocks) {
    kq_internal_set_error("bad channel/block");
    return -1;
  }
  if (b->g.pl_n <= 0 || !b->pl.plout) {
    kq_internal_set_error("no PL samples: the PL measurement is off (pl_tone_off, or N/decimate / 32 is no size with a transform)");
    return -1;
  }
  if (b->chans[ch].cfg.demod_type != KQ_FM_DEMOD) {
    kq_internal_set_error("no PL samples: channel %d is not an FM channel", ch);
    return -1;
  }
  if (cap < (size_t)b->g.pl_l) {
    kq_internal_set_error("PL sample buffer too small: %d > %zu", b->g.pl_l, cap);
    return -1;
  }
  if (sync_all(b)) return -1;
  KQ_TRY(hipMemcpy(dst, b->pl.plout + ((size_t)ch * b->g.max_blocks + blk) * b->g.pl_l, b->g.pl_l * sizeof(float),
                    hipMemcpyDeviceToHost));
  if (n) *n = (size_t)b->g.pl_l;
  return 0;
}

int kq_bank_pull_spectrum(kq_bank *b, int ch, unsigned blk, float *dst, size_t cap) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || cap < (size_t)b->g.N) {
    kq_internal_set_error("bad channel/capacity");
    return -1;
  }
  if (b->fwd_mode != KQ_FWD_FULL) {
    kq_internal_set_error("master spectrum exists only in KQ_FWD_FULL mode");
    return -1;
  }
  // The dump is armed for one channel at a time: the first pull after (re)arming returns -1 with a
  // hint; spectra are captured by the next kq_bank_process call.
  if (b->spec_ch != ch || !b->spec_dump) {
    if (!b->spec_dump && alloc_cleared(b, &b->spec_dump, (size_t)b->g.max_blocks * b->g.N)) return -1;
    b->spec_ch = ch;
    kq_internal_set_error("spectrum capture armed for channel %d; it is filled by the next process call", ch);
    return -1;
  }
  if (blk >= b->last_blocks) {
    kq_internal_set_error("bad block");
    return -1;
  }
  if (sync_all(b)) return -1;
  KQ_TRY(hipMemcpy(dst, b->spec_dump + (size_t)blk * b->g.N, b->g.N * sizeof(float2), hipMemcpyDeviceToHost));
  return 0;
}

int kq_bank_get_response(kq_bank *b, int ch, float *dst, size_t cap) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst || cap < (size_t)b->g.Ndec) {
    kq_internal_set_error("bad channel/capacity");
    return -1;
  }
  if (fetch_response(b, ch)) return -1;
  memcpy(dst, b->chans[ch].resp.data(), sizeof(float2) * b->g.Ndec);
  return 0;
}

int kq_bank_get_audio_response(kq_bank *b, int ch, float *dst, size_t cap) {
  BankScope dev_scope_(b);
  if (!valid_ch(b, ch) || !dst) {
    kq_internal_set_error("bad channel");
    return -1;
  }
  auto const &a = b->chans[ch].aresp;
  if (a.empty() || cap < a.size()) {
    kq_internal_set_error("no audio response (not FM, or flat) or capacity too small");
    return -1;
  }
  memcpy(dst, a.data(), sizeof(float2) * a.size());
  return 0;
}

}  // extern "C"
