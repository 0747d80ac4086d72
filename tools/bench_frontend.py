"""Throughput of the raw A/D conditioning stage (kq_fe_*) in front of the half-band cascade, device-resident.

python tools/bench_frontend.py [--log 6] [--out 1048576] [--block 131072] [--format s8] [--steps 50] [--kernels]

Three cases on the same raw stream, one JSON line each:
  a  kq_fe_process_decim: moments, scan, and the cascade reading the raw samples (2 B x n twice + 12 B x n_out)
  b  kq_fe_process to cf32, then kq_decim_process (2 B x n twice + 8 B x n written + 8 B x n read + 12 B x n_out)
  c  kq_decim_process alone on cf32, as tools/bench_decim.py measures it (8 B x n + 12 B x n_out)
--kernels reruns each case in a child process under `rocprofv3 --kernel-trace --stats` and adds the per-kernel average
times (a run of its own: the timings above are taken without the profiler).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def run_case(a, case):
    import numpy as np
    import torch
    from ka9q_sdr_amd import Decimator, FrontEnd, KQ_FE_S8, KQ_FE_S16
    fmt = KQ_FE_S16 if a.format == "s16" else KQ_FE_S8
    n = a.out << a.log
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    full = 32767 if fmt == KQ_FE_S16 else 127
    raw_h = np.clip(np.round(rng.standard_normal((n, 2)) * 0.05 * full + 0.01 * full), -full, full)
    raw = torch.from_numpy(raw_h.astype(np.int16 if fmt == KQ_FE_S16 else np.int8)).cuda()
    x = torch.randn(n, 2, device="cuda", dtype=torch.float32) * 0.05
    y = torch.empty(a.out, 2, device="cuda", dtype=torch.float32)
    s16 = torch.empty(a.out, 2, device="cuda", dtype=torch.int16)
    e = torch.zeros(1, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    fe = FrontEnd(fmt, a.block, 20e6, max_samples=n, stream=stream.cuda_stream,
                  decimator=dict(log_decimate=a.log, stage_threshold=a.thr, offset=1))
    dec = fe.decimator
    bps = 4 if fmt == KQ_FE_S16 else 2
    if case == "a":
        def call():
            fe.process_decim_device(raw.data_ptr(), a.out, y.data_ptr(), s16.data_ptr(), e.data_ptr())
        alg = 2.0 * bps * n + 12.0 * a.out
    elif case == "b":
        def call():
            fe.process_device(raw.data_ptr(), n, x.data_ptr())
            dec.process_device(x.data_ptr(), a.out, y.data_ptr(), s16.data_ptr(), e.data_ptr())
        alg = 2.0 * bps * n + 16.0 * n + 12.0 * a.out
    else:
        def call():
            dec.process_device(x.data_ptr(), a.out, y.data_ptr(), s16.data_ptr(), e.data_ptr())
        alg = 8.0 * n + 12.0 * a.out
    for _ in range(a.warmup):
        call()
    fe.sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(a.steps):
        call()
    t1.record(stream)
    fe.sync()
    ms = t0.elapsed_time(t1) / a.steps
    fe.close()
    return {"case": case, "metric": "raw samples conditioned and decimated per second" if case != "c" else
            "front-end samples decimated per second", "value": n / (ms * 1e-3), "unit": "complex samples/s",
            "ms_per_call": ms, "format": a.format, "block": a.block, "log_decimate": a.log, "n_out": a.out,
            "roofline": {"bound": "hbm", "bytes": alg, "achieved": alg / (ms * 1e-3) / 1e9, "peak": 8000.0,
                         "unit": "GB/s", "frac": alg / (ms * 1e-3) / 8e12}}


def kernel_stats(a, case):
    """per-kernel average time of one case from a profiled child process"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "fe", "--", sys.executable,
               os.path.abspath(__file__), "--case", case, "--log", str(a.log), "--thr", str(a.thr), "--out", str(a.out),
               "--block", str(a.block), "--format", a.format, "--steps", str(min(a.steps, 20)), "--warmup", "20"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"]
                if "k_fe_" in name or "k_hb_group" in name:
                    out[name.split("(")[0][-60:]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=6)
    ap.add_argument("--thr", type=int, default=8)
    ap.add_argument("--out", type=int, default=1 << 20)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--format", choices=["s8", "s16"], default="s8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200, help="untimed calls, to be at sustained clocks")
    ap.add_argument("--case", choices=["a", "b", "c"], help="one case only")
    ap.add_argument("--kernels", action="store_true", help="add per-kernel times from a rocprofv3 rerun")
    a = ap.parse_args()
    for case in ([a.case] if a.case else ["a", "b", "c"]):
        res = run_case(a, case)
        if a.kernels:
            res["kernels"] = kernel_stats(a, case)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
