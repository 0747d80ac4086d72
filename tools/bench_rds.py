"""Throughput of the RDS decoder bank (kq_rds_*) on device-resident composites.

python tools/bench_rds.py [--steps 20] [--warmup 5] [--no-split] [--no-wfm]
Rows: the decoder with 1, 128 and 1024 slots at Fc = 384 kHz, Dr = 16 (L = 2048, M = 2049, N = 4096; 8 frames = 16384
composite samples per call), and, as the yardstick for k_rds_front, the FM stereo decoder (kq_wfm_*) with 1024 slots on
the same frames (Da = 8: k_wfm_pilot runs two N-point transforms per frame, k_rds_front one and one of N / 16).  Prints one
JSON line per row: ms per call (median of per-call HIP event times), x real time, and the device ms per call of each
kernel from the same run repeated in a child process under rocprofv3 --kernel-trace --stats (null without it).
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

FC, DR, DA, L, M, FRAMES = 384000, 16, 8, 2048, 2049, 8
KERNELS = ("k_rds_ingest", "k_rds_front", "k_rds_track", "k_wfm_ingest", "k_wfm_pilot", "k_wfm_flags", "k_wfm_audio")


def _timed(bank, call, stream, steps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        call()
    bank.sync()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record(stream)
        call()
        e1.record(stream)
    bank.sync()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def rds(slots, steps, warmup):
    import torch
    from ka9q_sdr_amd.rds import RdsBank, rds_params
    n = FRAMES * L
    stream = torch.cuda.Stream()
    comp = (0.3 * torch.randn((slots, n), dtype=torch.float32, device="cuda")).contiguous()
    torch.cuda.synchronize()
    bank = RdsBank(FC, DR, L, M, max_slots=slots, max_samples=n, stream=stream.cuda_stream)
    cap = bank.max_groups(n)
    groups = torch.empty((slots, cap, 4), dtype=torch.int32, device="cuda")
    counts = torch.empty((slots,), dtype=torch.int32, device="cuda")
    st = torch.empty((slots, FRAMES, 6), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for s in range(slots):
        bank.set(s, rds_params(source=s))

    def call():
        assert bank.process_device(comp.data_ptr(), n, n, n, 1, groups.data_ptr(), cap, counts.data_ptr(), st.data_ptr(),
                                   FRAMES) == FRAMES

    ms = _timed(bank, call, stream, steps, warmup)
    bank.close()
    return dict(row="rds", slots=slots, samples_per_call=n, ms_per_call=round(ms, 4), x_realtime=round(n / FC * 1e3 / ms, 2))


def wfm(slots, steps, warmup):
    import torch
    from ka9q_sdr_amd.wfm import WfmBank, wfm_params
    n = FRAMES * L
    stream = torch.cuda.Stream()
    comp = (0.3 * torch.randn((slots, n), dtype=torch.float32, device="cuda")).contiguous()
    out = torch.empty((slots, 2 * n // DA), dtype=torch.float32, device="cuda")
    st = torch.empty((slots, FRAMES, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bank = WfmBank(FC, DA, L, M, max_slots=slots, max_samples=n, stream=stream.cuda_stream)
    for s in range(slots):
        bank.set(s, wfm_params(source=s))

    def call():
        assert bank.process_device(comp.data_ptr(), n, n, n, 1, out.data_ptr(), 2 * n // DA, st.data_ptr(), FRAMES) == FRAMES

    ms = _timed(bank, call, stream, steps, warmup)
    bank.close()
    return dict(row="wfm", slots=slots, samples_per_call=n, ms_per_call=round(ms, 4), x_realtime=round(n / FC * 1e3 / ms, 2))


def kernel_split(args, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rds", "--",
               sys.executable, os.path.abspath(__file__), "--child", args, str(steps), str(warmup)]
        try:
            if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode != 0:
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
    kind, slots = which.split(":")
    return (wfm if kind == "wfm" else rds)(int(slots), steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--no-wfm", action="store_true", help="skip the kq_wfm yardstick row")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        one(a.child[0], int(a.child[1]), int(a.child[2]))
        return
    rows = ["rds:1", "rds:128", "rds:1024"] + ([] if a.no_wfm else ["wfm:1024"])
    for w in rows:
        r = one(w, a.steps, a.warmup)
        if not a.no_split:
            r["device_ms"] = kernel_split(w, a.steps, a.warmup)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
