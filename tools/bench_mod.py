"""Throughput of the modulator bank (kq_mod_*) on device-resident audio and output.

python tools/bench_mod.py [--steps 50] [--warmup 20] [--max-realtime] [--only wide|ref1|ref4096] [--no-split]
Prints one JSON line per run: stations, geometry, ms per call (max_blocks blocks), G station-samples/s (output samples
times stations), x real time, the bytes a call moves to and from memory (audio in, group partials out and back in,
cf32 + int16 out), and the device time per call of k_mod_synth and k_mod_reduce.  Whole calls are timed with HIP events;
the split comes from the same run repeated in a child process under rocprofv3 --kernel-trace --stats (null without it).
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

GEOMS = {"wide": dict(samprate=10000000, L=8192, M=8193, interp=256),
         "ref": dict(samprate=192000, L=4096, M=4097, interp=4)}


def run(geom, stations, nblocks, steps, warmup):
    import numpy as np
    import torch
    import ka9q_sdr_amd as kq
    from ka9q_sdr_amd.modulate import KQ_PCM_S16
    g = GEOMS[geom]
    La = g["L"] // g["interp"]
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    pcm = torch.randint(-8000, 8000, (stations, nblocks * La), dtype=torch.int16, device="cuda")
    out = torch.empty(nblocks * g["L"], 2, dtype=torch.float32, device="cuda")
    s16 = torch.empty(nblocks * g["L"], 2, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    bank = kq.ModBank(max_stations=stations, max_blocks=nblocks, stream=stream.cuda_stream, **g)
    modes = ["am", "usb", "lsb", "ame", "fm"]
    for s in range(stations):
        bank.set_station(s, kq.station_config(modes[s % 5], frequency=float(rng.uniform(-0.45, 0.45) * g["samprate"]),
                                              amplitude_dbfs=-60.0, sweep=100.0 if s % 7 == 3 else 0.0))

    def call():
        bank.process_device(pcm.data_ptr(), KQ_PCM_S16, nblocks * La, nblocks, out.data_ptr(), s16.data_ptr())

    for _ in range(warmup):
        call()
    bank.sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(steps):
        call()
    t1.record(stream)
    bank.sync()
    ms = t0.elapsed_time(t1) / steps
    bank.close()
    samples = nblocks * g["L"]
    groups = -(-stations // -(-stations // 256))
    nbytes = stations * nblocks * La * 2 + 2 * groups * samples * 8 + samples * (8 + 4)
    return dict(stations=stations, geometry=dict(g, max_blocks=nblocks), ms_per_call=round(ms, 4),
                gsps=round(stations * samples / ms / 1e6, 2), x_realtime=round(samples / g["samprate"] * 1e3 / ms, 2),
                bytes_per_call=nbytes, gbps=round(nbytes / ms / 1e6, 1))


def kernel_split(geom, stations, nblocks, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mod", "--",
               sys.executable, os.path.abspath(__file__), "--child", geom, str(stations), str(nblocks), str(steps), str(warmup)]
        if subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode != 0:
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in ("k_mod_synth", "k_mod_reduce"):
                    if k in row.get("Name", ""):
                        out[k + "_ms"] = round(float(row["AverageNs"]) / 1e6, 4)
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--max-realtime", action="store_true", help="also: the largest station count at >= 1.0x real time (10 MS/s)")
    ap.add_argument("--only", choices=["wide", "ref1", "ref4096"], default=None)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--child", nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        geom, s, nb, steps, warmup = a.child[0], *map(int, a.child[1:])
        run(geom, s, nb, steps, warmup)
        return

    def report(r, geom, s, nb, steps, warmup):
        if not a.no_split:
            r["device_ms"] = kernel_split(geom, s, nb, steps, warmup)
        print(json.dumps(r), flush=True)

    runs = [("wide", 1024, 8), ("ref", 1, 8), ("ref", 4096, 8)]
    if a.only:
        runs = [dict(wide=runs[0], ref1=runs[1], ref4096=runs[2])[a.only]]
    for geom, s, nb in runs:
        report(run(geom, s, nb, a.steps, a.warmup), geom, s, nb, a.steps, a.warmup)
    if a.max_realtime:
        lo, hi = 1024, 1024
        while run("wide", hi, 8, 10, 3)["x_realtime"] >= 1.0 and hi < 65536:
            lo, hi = hi, min(65536, hi * 2)
        while hi - lo > max(64, lo // 32):
            mid = (lo + hi) // 2
            if run("wide", mid, 8, 10, 3)["x_realtime"] >= 1.0:
                lo = mid
            else:
                hi = mid
        r = run("wide", lo, 8, a.steps, a.warmup)
        r["max_realtime_stations"] = lo
        report(r, "wide", lo, 8, a.steps, a.warmup)


if __name__ == "__main__":
    main()
