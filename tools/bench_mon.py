"""Cost of the monitor mixer bank (kq_mon_*) on device-resident audio.

python tools/bench_mon.py [--steps 30] [--warmup 10] [--no-split]
Rows: 1 024, 8 192 and 34 560 mono sessions (random gains and positions, so the delayed sides read the history) in one bus
and spread over 16 buses, each at T = 64 frames (cfg 4's call: two blocks of 32 in a receiver bank's plane layout) and at
T = 960 (one block), float input, out + pcm + status written, 39 062 frames per second (10 MS/s / 256: H = 39).  Prints
one JSON line per row: ms per call (median of per-call HIP event times), its share of the 1.6384 ms call period, as the
yardstick a device-to-device hipMemcpyAsync of the bytes the call reads (sessions x T x 4) timed the same way in the same
run, and the device ms per call of each kernel from the same run repeated in a child process under rocprofv3
--kernel-trace --stats (null without it).
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

RATE, PERIOD_MS = 39062, 1.6384
KERNELS = ("k_mon_mix", "k_mon_reduce", "k_mon_status", "k_mon_hist")
SHAPES = {64: (32, 2), 960: (960, 1)}     # T: (block_len, nblocks)


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


def mon(sessions, buses, T, steps, warmup):
    import numpy as np
    import torch
    from ka9q_sdr_amd.monitor import KQ_MON_F32, MonBank
    block_len, nblocks = SHAPES[T]
    row_stride = 2 * block_len if nblocks > 1 else block_len      # a receiver bank's plane: [channel][block][2 olen]
    src_stride = nblocks * row_stride
    stream = torch.cuda.Stream()
    plane = (0.05 * torch.randn((sessions, src_stride), dtype=torch.float32, device="cuda")).contiguous()
    out = torch.empty((buses, T, 2), dtype=torch.float32, device="cuda")
    pcm = torch.empty((buses, T, 2), dtype=torch.int16, device="cuda")
    st = torch.empty((buses, 5), dtype=torch.int32, device="cuda")
    src = torch.empty((sessions, T), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    bank = MonBank(RATE, sessions, buses, T, stream=stream.cuda_stream)
    rng = np.random.default_rng(1)
    for s in range(sessions):
        bank.set(s, source=s, bus=s % buses, gain=float(rng.uniform(0, 2)), pan=float(rng.uniform(-1, 1)))

    def call():
        assert bank.process_device(plane.data_ptr(), KQ_MON_F32, src_stride, row_stride, block_len, nblocks, out.data_ptr(), 2 * T,
                                   pcm.data_ptr(), 2 * T, st.data_ptr()) == T

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    ms = _timed(call, bank.sync, stream, steps, warmup)
    copy_ms = _timed(copy, stream.synchronize, stream, steps, warmup)
    bank.close()
    return dict(row="mon", sessions=sessions, buses=buses, T=T, ms_per_call=round(ms, 4), share_of_period=round(ms / PERIOD_MS, 4),
                bytes_read=sessions * T * 4, copy_ms=round(copy_ms, 4), copy_share_of_period=round(copy_ms / PERIOD_MS, 4))


def kernel_split(args, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mon", "--",
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
    sessions, buses, T = (int(v) for v in which.split(":"))
    return mon(sessions, buses, T, steps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--rows", default=None, help="comma-separated sessions:buses:T instead of the standard table")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        one(a.child[0], int(a.child[1]), int(a.child[2]))
        return
    rows = a.rows.split(",") if a.rows else ["%d:%d:%d" % (s, b, T) for b in (1, 16) for s in (1024, 8192, 34560) for T in (64, 960)]
    for w in rows:
        r = one(w, a.steps, a.warmup)
        if not a.no_split:
            r["device_ms"] = kernel_split(w, a.steps, a.warmup)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
