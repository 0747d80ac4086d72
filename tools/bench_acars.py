"""Throughput of the ACARS decoder bank (kq_acars_*) on device-resident audio, beside kq_fsk_process at the same sample
rate on the same plane in the same run as the yardstick (a bank the parent commit has; it reads the plane as 2400 bit/s
baseband FSK with a low-pass of 21 taps, which costs it the same whatever the plane holds).

python tools/bench_acars.py [--steps 200] [--warmup 20] [--slots 4096] [--no-split]
Rows: Fs = 12 000 and 48 000 Hz (5 and 20 samples per bit), each in calls of 80 samples (a receiver's 1.6384 ms call at
configuration 4) and of 4096 samples; input and status on the device.  The input is a plane of 65536 samples per slot that
holds ACARS blocks from arinc618.modulate (amplitude 0.3, about two thirds of the time on the air) with noise of its own on
every slot, and the calls walk along it and start over, so the decoder finds syncs, walks open blocks and files them.  The
two banks are timed in turn, three times over, and every time is printed, so the spread of a run shows beside the
difference.
Prints one JSON line per row: ms per call (median of per-call HIP event times) of each repeat and their median, that
median as a fraction of the 1.6384 ms call period, and the device ms per call of each kernel from the same run repeated
in a child process under rocprofv3 --kernel-trace --stats, with no counters (null without it).
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

RATES = (12000, 48000)
CALLS = (80, 4096)
PLANE = 16 * 4096                                     # samples a slot's row holds; the calls walk along it
REPEATS = 3
CALL_PERIOD_MS = 1.6384                               # configuration 4: 80 samples at 48 828.125 Hz
KERNELS = ("k_acars", "k_fsk_front", "k_fsk_track")
FSK_TAPS = 21


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


def _input(fs, slots):
    """[slots][PLANE]: blocks of 60 characters of text one behind the other with gaps of half a block (amplitude 0.3),
    noise of its own (sigma 0.02) on each row"""
    import numpy as np
    import torch
    from ka9q_sdr_amd import arinc618
    blocks = [arinc618.encode_block(text=("POS N4012 W07401 FL350 ETA 1432 FOB 0123 %02d " % i * 2)[:60], block_id=str(i % 10))
              for i in range(64)]
    per_block = (64 + 40 + 8 * (len(blocks[0]) + 1) + 8) * fs // 2400
    row = arinc618.modulate(blocks[:PLANE // (per_block * 3 // 2) or 1], fs, amp=0.3, lead=per_block // 4, gap=per_block // 2)[:PLANE]
    row = np.concatenate([row, np.zeros(PLANE - len(row), np.float32)])
    x = torch.from_numpy(row).cuda()[None, :] + 0.02 * torch.randn((slots, PLANE), dtype=torch.float32, device="cuda")
    return x.contiguous()


def _walker(process, x, n):
    """a call that takes the plane's next n samples, and starts over at its end"""
    at = [0]
    base, rowbytes = x.data_ptr(), 4

    def call():
        process(base + rowbytes * at[0], n)
        at[0] = (at[0] + n) % (PLANE - PLANE % n)

    return call


def _bank(kind, fs, slots, n, stream):
    if kind == "acars":
        from ka9q_sdr_amd.acars import AcarsBank, acars_params
        bank = AcarsBank(float(fs), slots, n, max_blocks=64, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, acars_params(source=s))
    else:
        from ka9q_sdr_amd.fsk import FskBank, fsk_params
        bank = FskBank(fs, 2400, FSK_TAPS, slots, n, input_scale=32767.0, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, fsk_params(source=s, scrambled=0))
    return bank


def measure(fs, slots, n, steps, warmup, only=None):
    import numpy as np
    import torch
    from ka9q_sdr_amd import acars, fsk
    stream = torch.cuda.Stream()
    x = _input(fs, slots)
    kinds = [k for k in ("acars", "fsk") if only in (None, k)]
    mods = dict(acars=acars, fsk=fsk)
    words = dict(acars=acars.STATUS_WORDS, fsk=fsk.STATUS_DTYPE.itemsize // 4)
    st = {k: torch.zeros((slots, words[k]), dtype=torch.int32, device="cuda") for k in kinds}
    torch.cuda.synchronize()
    banks = {k: _bank(k, fs, slots, n, stream) for k in kinds}
    process = {k: (lambda p, m, k=k: banks[k].process_device(p, PLANE, m, m, 1, st[k].data_ptr(), 1)) for k in kinds}
    ms = {k: [] for k in kinds}
    for _ in range(REPEATS if only is None else 1):
        for k in kinds:                                    # in turn: what drifts during the run meets both alike
            ms[k].append(_timed(banks[k].sync, _walker(process[k], x, n), stream, steps, warmup))
    rows = []
    for k in kinds:
        med = float(np.median(ms[k]))
        r = dict(row=k, samprate=fs, slots=slots, samples_per_call=n, ms_per_call=round(med, 4), repeats=[round(t, 4) for t in ms[k]],
                 x_realtime=round(n / fs * 1e3 / med, 2), of_call_period=round(med / CALL_PERIOD_MS, 4))
        s = mods[k].status_array(st[k])
        if k == "acars":                                   # the decoder did find traffic
            r["syncs_per_slot"] = float(s["syncs"].mean())
            r["blocks_good_per_slot"] = float(s["blocks_good"].mean())
        else:
            r["bits_per_slot"] = float(s["bits"].mean())
        rows.append(r)
        banks[k].close()
    return rows


def kernel_split(which, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "acars", "--",
               sys.executable, os.path.abspath(__file__), "--child", which, str(steps), str(warmup)]
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
                m = re.search(r"\b(k_\w+)", row.get("Name", ""))   # past the namespaces and "void "
                if m and m.group(1) in KERNELS:
                    key = m.group(1) + "_ms"
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / calls / 1e6, 4)
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--rates", type=int, nargs="*", default=list(RATES))
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace reruns that split device time by kernel")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, fs, slots, n = a.child[0].split(":")
        measure(int(fs), int(slots), int(n), int(a.child[1]), int(a.child[2]), only=kind)
        return
    for fs in a.rates:
        for n in CALLS:
            for r in measure(fs, a.slots, n, a.steps, a.warmup):
                if not a.no_split:
                    r["device_ms"] = kernel_split("%s:%d:%d:%d" % (r["row"], fs, a.slots, n), a.steps, a.warmup)
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
