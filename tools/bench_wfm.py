"""Throughput of the FM stereo decoder bank (kq_wfm_*) on device-resident composites.

python tools/bench_wfm.py [--steps 20] [--warmup 5] [--only alone|chain] [--no-split]
Rows: the decoder alone with 1, 128 and 1024 slots at Fc = 384 kHz, Da = 8 (L = 6144, M = 2049, N = 8192; 8 frames =
49152 composite samples per call); the chain: a receiver bank of 128 flat FM channels at 12.288 MS/s (L = 8192,
M = 8193, D = 32: Fc = 384 kHz) and the decoder on its stream, 48 blocks (12288 composite samples) per call.  Prints one
JSON line per row: ms per call (alone: median of per-call HIP event times; chain: wall time of `steps` calls back to back
and one wait, median of three), x real time, and the device ms per call of each kernel from the same run repeated in a
child process under rocprofv3 --kernel-trace --stats (null without it).
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
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FC, DA, L, M = 384000, 8, 6144, 2049
FS, LB, MB, DRX, PER_CALL = 12288000, 8192, 8193, 32, 48
KERNELS = ("k_wfm_ingest", "k_wfm_pilot", "k_wfm_flags", "k_wfm_audio", "k_filter", "k_demod", "k_fm", "k_ingest")


def alone(slots, steps, warmup):
    import numpy as np
    import torch
    from ka9q_sdr_amd.wfm import WfmBank, wfm_params
    n = 8 * L
    stream = torch.cuda.Stream()
    comp = (0.3 * torch.randn((slots, n), dtype=torch.float32, device="cuda")).contiguous()
    out = torch.empty((slots, 2 * n // DA), dtype=torch.float32, device="cuda")
    st = torch.empty((slots, 8, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bank = WfmBank(FC, DA, L, M, max_slots=slots, max_samples=n, stream=stream.cuda_stream)
    for s in range(slots):
        bank.set(s, wfm_params(source=s))

    def call():
        assert bank.process_device(comp.data_ptr(), n, n, n, 1, out.data_ptr(), 2 * n // DA, st.data_ptr(), 8) == 8

    for _ in range(warmup):
        call()
    bank.sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record(stream)
        call()
        e1.record(stream)
    bank.sync()
    ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
    bank.close()
    return dict(row="alone", slots=slots, samples_per_call=n, ms_per_call=round(ms, 4), x_realtime=round(n / FC * 1e3 / ms, 2))


def chain(steps, warmup):
    import numpy as np
    import torch
    import ka9q_sdr_amd as kq
    from ka9q_sdr_amd.wfm import WfmBank, wfm_params
    C = 128
    rx = kq.Bank(FS, LB, MB, DRX, C, PER_CALL)
    for c in range(C):
        rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-150000.0, high=150000.0, flat=1,
                                         second_lo=-5.9e6 + c * 92000.0))
    wfm = WfmBank.beside(rx, DA, L, M, max_slots=C)
    for c in range(C):
        wfm.set(c, wfm_params(source=c))
    n = PER_CALL * LB
    iq = (torch.randn((n,), dtype=torch.complex64, device="cuda") * 0.05).contiguous()
    fmax = (PER_CALL * rx.olen + L - 1) // L
    out = torch.zeros((C, fmax * L // DA, 2), dtype=torch.float32, device="cuda")
    st = torch.zeros((C, fmax, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call():
        rx.push_iq_device(iq.data_ptr(), n)
        assert rx.process() == PER_CALL
        wfm.process_bank(rx, out, st)

    for _ in range(warmup):
        call()
    wfm.sync()
    reps = []
    for _ in range(3):   # calls back to back as a receiver runs them, then one wait: the throughput of the pair
        t0 = time.perf_counter()
        for _ in range(steps):
            call()
        wfm.sync()
        reps.append((time.perf_counter() - t0) / steps)
    ms = float(np.median(reps)) * 1e3
    wfm.close()
    rx.close()
    return dict(row="chain", channels=C, iq_samples_per_call=n, ms_per_call=round(ms, 4),
                x_realtime=round(n / FS * 1e3 / ms, 2))


def kernel_split(args, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "wfm", "--",
               sys.executable, os.path.abspath(__file__), "--child", args, str(steps), str(warmup)]
        try:
            if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode != 0:
                return None
        except subprocess.TimeoutExpired:
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        calls = steps * (3 if args == "chain" else 1) + warmup
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                m = re.search(r"\b(k_\w+)", row.get("Name", ""))   # past "(anonymous namespace)::" and "void "
                if m and m.group(1).startswith(KERNELS):
                    key = m.group(1) + "_ms"
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / calls / 1e6, 4)
        return out or None


def one(which, steps, warmup):
    return chain(steps, warmup) if which == "chain" else alone(int(which), steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["alone", "chain"], default=None)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        one(a.child[0], int(a.child[1]), int(a.child[2]))
        return
    rows = []
    if a.only in (None, "alone"):
        rows += ["1", "128", "1024"]
    if a.only in (None, "chain"):
        rows += ["chain"]
    for w in rows:
        r = one(w, a.steps, a.warmup)
        if not a.no_split:
            r["device_ms"] = kernel_split(w, a.steps, a.warmup)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
