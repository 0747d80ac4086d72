"""Throughput of the NAVTEX decoder bank (kq_navtex_*) on device-resident audio, beside kq_dsc_process on the same plane in
the same run as the yardstick (a bank the parent commit has).  Both read the plane at 1785 / 1615 Hz in frames of 12 samples at
100 baud, and their front halves and bit clocks are the same code -- two correlators, a window of ten frames, the three-point
clock -- so the difference is the tracker's above the bit: k_dsc's ten-bit symbols and open message against k_navtex's
seven-bit places, its two sync attempts and an event per character.  The two banks do different work on the plane: it holds
NAVTEX traffic, on which k_dsc's tracker finds no phasing sequence and files nothing, while k_navtex files seven events a
second per slot.

python tools/bench_navtex.py [--steps 200] [--warmup 20] [--slots 4096 16384] [--no-split]
Rows: Fs = 12 kHz, B = 12 (frames of 1 ms, 10 to a bit of 100 baud), in calls of 1200 samples and of 4096 samples (341 ms of
signal); input and status on the device.  The input is a plane of 65536 samples per slot that holds a NAVTEX message of
24 characters behind six phasing pairs from ccir476.modulate with noise of its own on every slot, and the calls walk along
it and start over, so the decoder reads the message once per pass; an arena holds 512 events, and once a long run has filled
it further events are counted as dropped, which costs the kernel the same branch.  The two banks are timed in turn, three
times over, and every time is printed, so the spread of a run shows beside the difference.
Prints one JSON line per row: ms per call (median of per-call HIP event times) of each repeat and their median, how many
times faster than the signal that is (x_realtime: samples_per_call / Fs over the median), and the device ms per call of
each kernel from the same run repeated in a child process under rocprofv3 --kernel-trace --stats, with no counters (null
without it).
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

FS = 12000
BLOCK = 12
BAUD, MARK, SPACE = 100.0, 1785.0, 1615.0
CALLS = (1200, 4096)
PLANE = 16 * 4096                                     # samples a slot's row holds; the calls walk along it
REPEATS = 3
KERNELS = ("k_navtex", "k_dsc")
KINDS = ("navtex", "dsc")


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


def _input(slots):
    """[slots][PLANE]: a NAVTEX message on every row (amplitude 0.3), noise of its own (sigma 0.02) on each"""
    import numpy as np
    import torch
    from ka9q_sdr_amd import ccir476
    codes = ccir476.codes_of("ZCZC FA01\r\nGALE\r\nNNNN")
    row = ccir476.modulate(ccir476.bits(ccir476.places(codes, phasing=(6, 1))), FS, BAUD, MARK, SPACE, 0.3)[:PLANE]
    row = np.concatenate([row, np.zeros(PLANE - len(row), np.float32)])
    x = torch.from_numpy(row).cuda()[None, :].repeat(slots, 1)
    for s0 in range(0, slots, 1024):                       # in parts: no second plane of noise beside the first
        x[s0:s0 + 1024] += 0.02 * torch.randn((min(1024, slots - s0), PLANE), dtype=torch.float32, device="cuda")
    return x.contiguous()


def _walker(process, x, n):
    """a call that takes the plane's next n samples, and starts over at its end"""
    at = [0]
    base, rowbytes = x.data_ptr(), 4

    def call():
        process(base + rowbytes * at[0], n)
        at[0] = (at[0] + n) % (PLANE - PLANE % n)

    return call


def _bank(kind, slots, n, stream):
    if kind == "navtex":
        from ka9q_sdr_amd.navtex import NavtexBank, navtex_params
        bank = NavtexBank(FS, BLOCK, slots, n, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, navtex_params(source=s, mark=MARK, space=SPACE, baud=BAUD))
    else:
        from ka9q_sdr_amd.dsc import DscBank, dsc_params
        bank = DscBank(FS, BLOCK, slots, n, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, dsc_params(source=s, mark=MARK, space=SPACE, baud=BAUD))
    return bank


def measure(slots, n, steps, warmup, only=None):
    import numpy as np
    import torch
    from ka9q_sdr_amd import dsc, navtex
    stream = torch.cuda.Stream()
    x = _input(slots)
    kinds = [k for k in KINDS if only in (None, k)]
    mods = dict(navtex=navtex, dsc=dsc)
    st = {k: torch.zeros((slots, mods[k].STATUS_WORDS), dtype=torch.int32, device="cuda") for k in kinds}
    torch.cuda.synchronize()
    banks = {k: _bank(k, slots, n, stream) for k in kinds}
    process = {k: (lambda p, m, k=k: banks[k].process_device(p, PLANE, m, m, 1, st[k].data_ptr(), 1)) for k in kinds}
    ms = {k: [] for k in kinds}
    for _ in range(REPEATS if only is None else 1):
        for k in kinds:                                    # in turn: what drifts during the run meets all alike
            ms[k].append(_timed(banks[k].sync, _walker(process[k], x, n), stream, steps, warmup))
    rows = []
    for k in kinds:
        med = float(np.median(ms[k]))
        r = dict(row=k, slots=slots, samples_per_call=n, ms_per_call=round(med, 4), repeats=[round(t, 4) for t in ms[k]],
                 x_realtime=round(n / FS * 1e3 / med, 2))
        r["events_per_slot"] = float(mods[k].status_array(st[k])["events"].mean())  # (navtex: the decoder did find traffic)
        rows.append(r)
        banks[k].close()
    return rows


def kernel_split(which, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "navtex", "--",
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
    ap.add_argument("--slots", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace reruns that split device time by kernel")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, slots, n = a.child[0].split(":")
        measure(int(slots), int(n), int(a.child[1]), int(a.child[2]), only=kind)
        return
    for slots in a.slots:
        for n in CALLS:
            for r in measure(slots, n, a.steps, a.warmup):
                if not a.no_split and r["row"] == "navtex":
                    r["device_ms"] = kernel_split("%s:%d:%d" % (r["row"], slots, n), a.steps, a.warmup)
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
