"""Throughput of the POCSAG pager decoder bank (kq_pag_*) on device-resident discriminator output, beside kq_fsk_process on
the same input and geometry in the same run (the two share their front end, k_fsk_front; the trackers differ).

python tools/bench_pag.py [--steps 50] [--warmup 10] [--slots 4096] [--no-split]
Rows: Fs = 48 kHz, 2400 bit/s (20 samples per bit), K = 41, W = 480, cutoff 0.75 baud, in calls of 80 samples (a receiver's
1.64 ms call) and of 4096 samples; inputs and status on the device.  The input is a plane of 65536 samples per slot that
holds a transmission of five batches from pocsag.encode, with its own noise on every slot, and the calls walk along it
and start over, so the pager tracker finds its batches and assembles pages; the packet tracker (unscrambled NRZI) sees
the same bits.  The two banks are timed in turn, three times over, and every time is printed, so the spread of a run
shows beside the difference.
Prints one JSON line per row: ms per call (median of per-call HIP event times) of each repeat and their median, and the
device ms per call of each kernel from the same run repeated in a child process under rocprofv3 --kernel-trace --stats
(null without it).
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

FS, BAUD, K, WINDOW_BITS = 48000, 2400, 41, 24.0      # W = 480
CALLS = (80, 4096)
PLANE = 16 * 4096                                     # samples a slot's row holds; the calls walk along it
REPEATS = 3
KERNELS = ("k_fsk_front", "k_fsk_track", "k_pag_track")


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
    """[slots][PLANE]: one transmission of five batches (0.3 rad/sample on a DC of 0.05) on every row, noise of its own
    (sigma 0.03) on each"""
    import numpy as np
    import torch
    from ka9q_sdr_amd import pocsag
    rng = np.random.default_rng(1)
    spb = FS // BAUD
    pages = []
    while len(pocsag.encode(pages, BAUD)[0]) <= 5 * 17:
        pages.append((int(rng.integers(8, 1 << 21)), int(rng.integers(0, 4)), [int(v) for v in rng.integers(0, 1 << 20, 6)]))
    bits = pocsag.encode(pages[:-1], BAUD)[1][pocsag.PREAMBLE_BITS - 64:]
    lv = np.repeat(2.0 * bits - 1.0, spb).astype(np.float32)
    assert len(lv) <= PLANE
    row = np.full(PLANE, 0.05, np.float32)
    row[:len(lv)] += 0.3 * lv
    x = torch.from_numpy(row).cuda()[None, :] + 0.03 * torch.randn((slots, PLANE), dtype=torch.float32, device="cuda")
    return x.contiguous()


def _walker(bank, x, n, st):
    """a call that takes the plane's next n samples, and starts over at its end"""
    at = [0]
    base, rowbytes = x.data_ptr(), 4

    def call():
        bank.process_device(base + rowbytes * at[0], PLANE, n, n, 1, st.data_ptr(), 1)
        at[0] = (at[0] + n) % (PLANE - PLANE % n)

    return call


def _bank(kind, slots, n, stream):
    if kind == "pag":
        from ka9q_sdr_amd.pag import PagBank, pag_params
        bank = PagBank(FS, BAUD, K, slots, n, window_bits=WINDOW_BITS, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, pag_params(source=s))
    else:
        from ka9q_sdr_amd.fsk import FskBank, fsk_params
        bank = FskBank(FS, BAUD, K, slots, n, cutoff_hz=0.75 * BAUD, window_bits=WINDOW_BITS, stream=stream.cuda_stream)
        for s in range(slots):
            bank.set(s, fsk_params(source=s, scrambled=0))
    return bank


def measure(slots, n, steps, warmup, only=None):
    import numpy as np
    import torch
    from ka9q_sdr_amd.pag import STATUS_WORDS, status_array
    stream = torch.cuda.Stream()
    x = _input(slots)
    width = {"pag": STATUS_WORDS, "fsk": 8}
    kinds = [k for k in ("pag", "fsk") if only in (None, k)]
    st = {k: torch.zeros((slots, width[k]), dtype=torch.int32, device="cuda") for k in kinds}
    torch.cuda.synchronize()
    banks = {k: _bank(k, slots, n, stream) for k in kinds}
    ms = {k: [] for k in kinds}
    for _ in range(REPEATS if only is None else 1):
        for k in kinds:                                    # in turn: what drifts during the run meets both alike
            ms[k].append(_timed(banks[k].sync, _walker(banks[k], x, n, st[k]), stream, steps, warmup))
    rows = []
    for k in kinds:
        med = float(np.median(ms[k]))
        r = dict(row=k, slots=slots, samples_per_call=n, ms_per_call=round(med, 4), repeats=[round(t, 4) for t in ms[k]],
                 x_realtime=round(n / FS * 1e3 / med, 2))
        if k == "pag":                                     # the tracker did find traffic: pages per slot so far
            r["pages_per_slot"] = float(status_array(st[k])["pages"].mean())
        rows.append(r)
        banks[k].close()
    return rows


def kernel_split(which, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pag", "--",
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
                if m and m.group(1).startswith(KERNELS):
                    key = m.group(1) + "_ms"
                    out[key] = round(out.get(key, 0.0) + float(row["TotalDurationNs"]) / calls / 1e6, 4)
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace reruns that split device time by kernel")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, slots, n = a.child[0].split(":")
        measure(int(slots), int(n), int(a.child[1]), int(a.child[2]), only=kind)
        return
    for n in CALLS:
        for r in measure(a.slots, n, a.steps, a.warmup):
            if not a.no_split:
                r["device_ms"] = kernel_split("%s:%d:%d" % (r["row"], a.slots, n), a.steps, a.warmup)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
