"""Cost of the rational resampler bank (kq_rsmp_*) on device-resident audio.

python tools/bench_rsmp.py [--steps 30] [--warmup 10]
Rows: 1 024 and 32 768 mono slots at 768 / 625 (39 062.5 -> 48 000 Hz: 10 MS/s / 256), T = 32 taps per phase, float input
in a receiver bank's plane layout, `out` written; each at 1 250 samples per slot and call (32 ms of audio, J = 1 536) and
at 64 (cfg 4's call: two blocks of 32).  Prints one JSON line per row: ms per call (median of per-call HIP event times),
slot-samples per second (input samples of all slots over that time), as the yardstick a device-to-device copy of the
bytes the call moves (what it reads plus what it writes, split evenly between the copy's two sides) timed the same way in
the same run, and the ratio of the two times.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NUM, DEN, FO, TAPS, BETA = 10000000, 256, 48000, 32, 3.0
SHAPES = {64: (32, 2), 1250: (1250, 1)}     # samples per call: (block_len, nblocks)


def _timed(call, sync, stream, steps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        call()
    sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record(stream)
        call()
        e1.record(stream)
    sync()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def rsmp(slots, n, steps, warmup):
    import torch
    from ka9q_sdr_amd.packet import KQ_PCM_F32
    from ka9q_sdr_amd.resample import RsmpBank
    block_len, nblocks = SHAPES[n]
    row_stride = 2 * block_len if nblocks > 1 else block_len      # a receiver bank's plane: [channel][block][2 olen]
    src_stride = nblocks * row_stride
    stream = torch.cuda.Stream()
    plane = (0.05 * torch.randn((slots, src_stride), dtype=torch.float32, device="cuda")).contiguous()
    bank = RsmpBank(NUM, DEN, FO, TAPS, RsmpBank.clean_cutoff(NUM / DEN, FO, TAPS, BETA), BETA, slots, n,
                    stream=stream.cuda_stream)
    width = bank.max_out(n)
    out = torch.empty((slots, width), dtype=torch.float32, device="cuda")
    moved = slots * (n + width) * 4                               # bytes read + bytes written, to within one output per slot
    src = torch.empty(moved // 8, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    for s in range(slots):
        bank.set(s, source=s, channels=1)

    def call():
        assert bank.process_device(plane.data_ptr(), KQ_PCM_F32, src_stride, row_stride, block_len, nblocks, out.data_ptr(),
                                   width) in (width - 1, width)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    ms = _timed(call, bank.sync, stream, steps, warmup)
    copy_ms = _timed(copy, stream.synchronize, stream, steps, warmup)
    bank.close()
    return dict(row="rsmp", slots=slots, samples_per_call=n, P=bank.P, Q=bank.Q, taps=TAPS, ms_per_call=round(ms, 4),
                slot_samples_per_s=round(slots * n / (ms * 1e-3)), realtime_slots=round(slots * n / (ms * 1e-3) / (NUM / DEN)),
                bytes_moved=moved, copy_ms=round(copy_ms, 4), ratio_to_copy=round(ms / copy_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", default=None, help="comma-separated slots:samples instead of the standard table")
    a = ap.parse_args()
    rows = a.rows.split(",") if a.rows else ["%d:%d" % (s, n) for s in (1024, 32768) for n in (1250, 64)]
    for w in rows:
        slots, n = (int(v) for v in w.split(":"))
        print(json.dumps(rsmp(slots, n, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
