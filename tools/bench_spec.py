"""Throughput of the spectrum bank (kq_spec_*) at 10 MS/s on device-resident int16 I/Q.

python tools/bench_spec.py [--steps 30] [--warmup 10] [--samples 1048576] [--only a|b|c] [--no-split]
Scenarios: (a) one 16384-bin overview (Dz 1, H Nf/2); (b) 256 zoom analyzers (Dz 64, Nf 4096, B 3072, H Nf/2); (c) both.
Prints one JSON line per scenario: ms per call (median of per-call HIP event times after warm-up), x real time, and the
device ms per call of each k_spec_* kernel, from the same run repeated in a child process under
rocprofv3 --kernel-trace --stats (null without it).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FS = 10000000
KERNELS = ("k_spec_ingest", "k_spec_decim", "k_spec_frames", "k_spec_rows")


def analyzers(scenario):
    from ka9q_sdr_amd.spectrum import spec_params
    out = []
    if scenario in ("a", "c"):
        out.append(spec_params(16384, hop=8192, average=4))
    if scenario in ("b", "c"):
        for i in range(256):
            out.append(spec_params(4096, bins=3072, decimate=64, hop=2048, average=4,
                                   center=-4.8e6 + i * 9.6e6 / 256, sweep=50.0 if i % 8 == 0 else 0.0))
    return out


def run(scenario, nsamples, steps, warmup):
    import numpy as np
    import torch
    from ka9q_sdr_amd.spectrum import KQ_IQ_S16, SpecBank
    stream = torch.cuda.Stream()
    iq = torch.randint(-3000, 3000, (nsamples, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    plist = analyzers(scenario)
    bank = SpecBank(FS, max_specs=len(plist), max_samples=nsamples, max_rows=1 << 16, stream=stream.cuda_stream)
    for s, p in enumerate(plist):
        bank.set(s, p)

    def call():
        bank.process_device(iq.data_ptr(), KQ_IQ_S16, nsamples)

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
    return dict(scenario=scenario, analyzers=len(plist), samples_per_call=nsamples, ms_per_call=round(ms, 4),
                x_realtime=round(nsamples / FS * 1e3 / ms, 2))


def kernel_split(scenario, nsamples, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "spec", "--",
               sys.executable, os.path.abspath(__file__), "--child", scenario, str(nsamples), str(steps), str(warmup)]
        if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode != 0:
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        calls = steps + warmup
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row.get("Name", ""):   # per call: the total over the run's calls (some kernels run per group)
                        out[k + "_ms"] = round(float(row["TotalDurationNs"]) / calls / 1e6, 4)
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run(a.child[0], *map(int, a.child[1:]))
        return
    for sc in ([a.only] if a.only else ["a", "b", "c"]):
        r = run(sc, a.samples, a.steps, a.warmup)
        if not a.no_split:
            r["device_ms"] = kernel_split(sc, a.samples, a.steps, a.warmup)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
