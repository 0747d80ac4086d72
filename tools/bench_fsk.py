"""Throughput of the FSK / GMSK packet decoder bank (kq_fsk_*) on device-resident discriminator output.

python tools/bench_fsk.py [--steps 50] [--warmup 10] [--no-split] [--no-yardsticks]
Rows: the decoder at Fs = 48 kHz, 9600 bit/s, K = 21, W = 80 with 1, 128, 1024 and 4096 slots, in calls of 80 samples (a
receiver's 1.64 ms call) and of 4096 samples; inputs and status on the device.  Yardsticks, timed the same way in the same
run: a device-to-device hipMemcpyAsync of the bytes the call reads (slots x samples x 4), and kq_afsk_push, the existing
packet decoder, on the same number of sessions and samples.  Prints one JSON line per row: ms per call (median of per-call
HIP event times), the share of a 1.6384 ms call period it takes where the call is 80 samples, and the device ms per call
of each kernel from the same run repeated in a child process under rocprofv3 --kernel-trace --stats (null without it).
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FS, BAUD, K, WINDOW_BITS = 48000, 9600, 21, 16.0     # W = 80
SLOTS = (1, 128, 1024, 4096)
CALLS = (80, 4096)
PERIOD_MS = 1.6384
KERNELS = ("k_fsk_front", "k_fsk_track", "k_afsk")


def _timed(sync, call, stream, steps, warmup):
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


def _input(slots, n):
    """noise around an alternating pattern: the clock has edges to follow and the deframer sees random bits"""
    import torch
    t = torch.arange(n, device="cuda") // 5 % 2
    x = (0.3 * (2.0 * t - 1.0))[None, :] + 0.2 * torch.randn((slots, n), dtype=torch.float32, device="cuda")
    return x.contiguous()


def _row(kind, slots, n, ms):
    r = dict(row=kind, slots=slots, samples_per_call=n, ms_per_call=round(ms, 4), x_realtime=round(n / FS * 1e3 / ms, 2))
    if n == 80:
        r["share_of_call_period"] = round(ms / PERIOD_MS, 4)
    return r


def fsk(slots, n, steps, warmup):
    import torch
    from ka9q_sdr_amd.fsk import FskBank, fsk_params
    stream = torch.cuda.Stream()
    x = _input(slots, n)
    st = torch.empty((slots, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bank = FskBank(FS, BAUD, K, slots, n, window_bits=WINDOW_BITS, stream=stream.cuda_stream)
    for s in range(slots):
        bank.set(s, fsk_params(source=s, scrambled=s % 2))
    ms = _timed(bank.sync, lambda: bank.process_device(x.data_ptr(), n, n, n, 1, st.data_ptr(), 1), stream, steps, warmup)
    bank.close()
    return _row("fsk", slots, n, ms)


def copy(slots, n, steps, warmup):
    import torch
    stream = torch.cuda.Stream()
    x = _input(slots, n)
    y = torch.empty_like(x)
    torch.cuda.synchronize()

    def call():
        with torch.cuda.stream(stream):
            y.copy_(x, non_blocking=True)      # hipMemcpyAsync, device to device

    ms = _timed(stream.synchronize, call, stream, steps, warmup)
    return _row("copy", slots, n, ms)


def afsk(slots, n, steps, warmup):
    import torch
    import ka9q_sdr_amd as kq
    stream = torch.cuda.Stream()
    x = _input(slots, n)
    torch.cuda.synchronize()
    bank = kq.AfskBank(slots, max_frames=4, stream=stream.cuda_stream)

    def call():
        bank.push_device(x.data_ptr(), n, n)

    ms = _timed(bank.sync, call, stream, steps, warmup)
    bank.close()
    return _row("afsk", slots, n, ms)


def kernel_split(args, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fsk", "--",
               sys.executable, os.path.abspath(__file__), "--child", args, str(steps), str(warmup)]
        try:
            if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300).returncode != 0:
                return None
        except subprocess.TimeoutExpired:
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        calls = steps + warmup
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                m = re.search(r"\b(k_\w+)", row.get("Name", ""))   # past "(anonymous namespace)::" and "void "
                if m and m.group(1).startswith(KERNELS):
                    key = m.group(1) + "_ms"
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / calls / 1e6, 4)
        return out or None


def one(which, steps, warmup):
    kind, slots, n = which.split(":")
    return dict(fsk=fsk, copy=copy, afsk=afsk)[kind](int(slots), int(n), steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--no-yardsticks", action="store_true", help="skip the copy and kq_afsk rows")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        one(a.child[0], int(a.child[1]), int(a.child[2]))
        return
    for n in CALLS:
        for slots in SLOTS:
            for kind in ("fsk",) if a.no_yardsticks else ("fsk", "copy", "afsk"):
                w = "%s:%d:%d" % (kind, slots, n)
                r = one(w, a.steps, a.warmup)
                if kind == "fsk" and not a.no_split:
                    r["device_ms"] = kernel_split(w, a.steps, a.warmup)
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
