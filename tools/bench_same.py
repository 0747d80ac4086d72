"""Throughput of the SAME decoder bank (kq_same_*) on device-resident audio, beside kq_navtex_process and kq_dsc_process on the
same plane in the same run as the yardsticks (banks the parent commit has).  All three read the plane at 2083.3 / 1562.5 Hz in
frames of 8 samples at 520.83 baud, and their front halves and bit clocks are the same code -- two correlators, a window of
twelve frames, the three-point clock -- so the difference is the tracker's above the bit: k_same's two 48-bit patterns and a
byte every eighth bit against k_navtex's and k_dsc's sync attempts.  The three banks do different work on the plane: it holds
SAME bursts, on which k_navtex and k_dsc find no sync and file nothing, while k_same files 40 events a burst per slot.
Each bank is entered twice, as two banks of the same kind with the same slots, so the spread between two entries that do
the same work (A/A) shows beside the difference between the kinds.

python tools/bench_same.py [--steps 200] [--warmup 20] [--slots 16384] [--no-split]
Rows: Fs = 48 kHz, B = 8 (11.52 frames to a bit), in calls of 4096 samples (85 ms of signal); input and status on the device.
The input is a plane of 65536 samples per slot (1.37 s) that holds one header burst of 58 bytes from eas.modulate with
noise of its own on every slot, and the calls walk along it and start over, so the decoder reads the burst once per pass; an
arena holds 512 events, and once a long run has filled it further events are counted as dropped, which costs the kernel the
same branch.  The six entries are timed in turn, three times over, and every time is printed.
Prints one JSON line per entry: ms per call (median of per-call HIP event times) of each repeat and their median, how many
times faster than the signal that is (x_realtime: samples_per_call / Fs over the median), and for the first entry of
kq_same_process the device ms per call of k_same from the same run repeated in a child process under rocprofv3
--kernel-trace --stats, with no counters (null without it).
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

FS = 48000
BLOCK = 8
BAUD, MARK, SPACE = 3125.0 / 6.0, 6250.0 / 3.0, 1562.5
CALLS = (4096,)
PLANE = 16 * 4096                                     # samples a slot's row holds; the calls walk along it
REPEATS = 3
KERNELS = ("k_same", "k_navtex", "k_dsc")
KINDS = ("same", "navtex", "dsc")
ENTRIES = tuple((k, e) for e in (1, 2) for k in KINDS)  # same, navtex, dsc, and again


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
    """[slots][PLANE]: a SAME header burst on every row (amplitude 0.3), noise of its own (sigma 0.02) on each"""
    import numpy as np
    import torch
    from ka9q_sdr_amd import eas
    text = eas.header("WXR", "RWT", [12345], "0015", "1231200", "KABC/FM")
    row = eas.modulate(text, FS, eom=False, repeats=1, amp=0.3, lead=0.1, tail=0.0)[:PLANE]
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


def _modules():
    from ka9q_sdr_amd import dsc, navtex, same
    return dict(same=(same, same.SameBank, same.same_params), navtex=(navtex, navtex.NavtexBank, navtex.navtex_params),
                dsc=(dsc, dsc.DscBank, dsc.dsc_params))


def _bank(kind, slots, n, stream):
    _, cls, params = _modules()[kind]
    bank = cls(FS, BLOCK, slots, n, stream=stream.cuda_stream, max_events=512)
    for s in range(slots):
        bank.set(s, params(source=s, mark=MARK, space=SPACE, baud=BAUD))
    return bank


def measure(slots, n, steps, warmup, only=None):
    import numpy as np
    import torch
    stream = torch.cuda.Stream()
    x = _input(slots)
    entries = [e for e in ENTRIES if only is None or e == (only, 1)]
    mods = {k: v[0] for k, v in _modules().items()}
    st = {e: torch.zeros((slots, mods[e[0]].STATUS_WORDS), dtype=torch.int32, device="cuda") for e in entries}
    torch.cuda.synchronize()
    banks = {e: _bank(e[0], slots, n, stream) for e in entries}
    process = {e: (lambda p, m, e=e: banks[e].process_device(p, PLANE, m, m, 1, st[e].data_ptr(), 1)) for e in entries}
    ms = {e: [] for e in entries}
    for _ in range(REPEATS if only is None else 1):
        for e in entries:                                  # in turn: what drifts during the run meets all alike
            ms[e].append(_timed(banks[e].sync, _walker(process[e], x, n), stream, steps, warmup))
    rows = []
    for e in entries:
        med = float(np.median(ms[e]))
        r = dict(row=e[0], entry=e[1], slots=slots, samples_per_call=n, ms_per_call=round(med, 4),
                 repeats=[round(t, 4) for t in ms[e]], x_realtime=round(n / FS * 1e3 / med, 2))
        r["events_per_slot"] = float(mods[e[0]].status_array(st[e])["events"].mean())  # (same: the decoder did find bursts)
        rows.append(r)
        banks[e].close()
    return rows


def kernel_split(which, steps, warmup):
    """device ms per call of each kernel: the run again in a child under rocprofv3's kernel trace"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "same", "--",
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
    ap.add_argument("--slots", type=int, nargs="+", default=[16384])
    ap.add_argument("--no-split", action="store_true", help="skip the kernel-trace rerun that splits device time by kernel")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, slots, n = a.child[0].split(":")
        measure(int(slots), int(n), int(a.child[1]), int(a.child[2]), only=kind)
        return
    for slots in a.slots:
        for n in CALLS:
            for r in measure(slots, n, a.steps, a.warmup):
                if not a.no_split and (r["row"], r["entry"]) == ("same", 1):
                    r["device_ms"] = kernel_split("%s:%d:%d" % (r["row"], slots, n), a.steps, a.warmup)
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
