"""The reference's decision-heavy loops running above this library, three ways on the same input:

  * the REFERENCE's own loop -- fm.c, linear.c, packet.c compiled where they lie, unmodified, against
    include/ka9q_hip_compat.h (oracle/Makefile -> oracle/_ref/libref_{fm,linear,packet}_dropin.so; built in the build
    container, travel prebuilt) -- on this library's filter, oscillator and fftwf_* calls on the GPU;
  * the library's own thread (demod_fm / demod_linear) or bank (kq_afsk_*);
  * the oracle chain.

A misreading of the reference that went into both the oracle and the kernels shows here as the first of the three leaving
the other two.  fm and linear above the library are boundary evidence (the filter under them is ours); the AFSK decode
loop, whose frames are byte-exact, is pinned.  Every bar is one the suite already holds for the same quantity
(test_gpu_dropin.py, test_gpu_parity.py::test_linear_carrier_pll, test_gpu_packet.py).

Every child runs under its own timeout; one that ends on a signal or on its timeout sets a module flag and the rest of the
module skips, so that nothing more is started on the card after a fault."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import kq_oracle as ko
from common import afsk_audio, afsk_bits, ax25_fcs, rel_rms
from test_gpu_dropin import FM, GEOMS, USB, _oracle, _run, _signal, harness  # noqa: F401  (harness is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = {m: os.path.join(ROOT, "oracle", "_ref", "libref_%s_dropin.so" % m) for m in ("fm", "linear", "packet")}
pytestmark = pytest.mark.gpu

G0 = (192000, 2048, 2049, 4)
G1 = (192000, 8192, 8193, 4)          # cfg 1
CHILD_TIMEOUT = 120
_FAULT = []                           # why the rest of the module skips
# what the HIP runtime and the driver say when a kernel has faulted the card, in lower case
_FAULT_TEXT = ("illegal memory access", "memory access fault", "hiperrorillegaladdress", "hiperrorlaunchfailure",
               "unspecified launch failure", "hsa_status_error", "gpu hang", "core dumped")


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    if _FAULT:
        pytest.skip("a child of this module ended on a signal or its timeout: " + _FAULT[0])


def _guard(what, fn, *a, **kw):
    """fn(...) is one child process on the card; a signal or a timeout there ends GPU work for this module"""
    try:
        return fn(*a, **kw)
    except subprocess.TimeoutExpired:
        _FAULT.append("%s: timeout" % what)
        raise
    except AssertionError as e:
        rc = getattr(fn, "last_rc", None)
        if rc is not None and (rc < 0 or rc in (124, 134, 137, 139)):
            _FAULT.append("%s: exit status %d" % (what, rc))
        elif rc:                  # an ordinary failure status: the child's own output (in the message) may still name a GPU fault
            said = str(e).lower()
            for sign in _FAULT_TEXT:
                if sign in said:
                    _FAULT.append("%s: exit status %d, output says '%s'" % (what, rc, sign))
                    break
        raise


def _need(mode):
    """the object travels prebuilt; it may be absent only where there is no reference tree to build it from"""
    if not os.path.exists(REF[mode]):
        if not os.path.isdir("/root/reference"):
            pytest.skip("oracle/_ref/libref_%s_dropin.so not built (needs the reference tree)" % mode)
        pytest.fail("the reference tree is present but build() did not make %s" % REF[mode])


def _three(exe, mode, iq, p, extra, geom, nb):
    """-> reference's loop on the library, the library's own thread, the oracle chain"""
    _need(mode)
    ex = list(extra) + ["--status12"]
    ref, rtail = _guard("reference %s.c" % mode, _run, exe, mode, iq, p["low"], p["high"], ex + ["--ref", REF[mode]], geom, nb, CHILD_TIMEOUT)
    mine, mtail = _guard("library demod_%s" % mode, _run, exe, mode, iq, p["low"], p["high"], ex, geom, nb, CHILD_TIMEOUT)
    auds, sts, filts = _oracle(p, iq, geom, nb, want_filt=True)
    return (ref, rtail), (mine, mtail), (auds, sts, filts)


def _cat(recs, first=0):
    return np.concatenate([a for a, _ in recs[first:]])


# ---------------------------------------------------------------- FM (fm.c:21-186)
def _fm_bars(ref, mine, sts, blocks, keys=("pdeviation", "foffset", "bb_power", "n0")):
    """the bars of test_library_demod_fm_thread and test_reference_am_c_runs_on_the_library"""
    bar = dict(pdeviation=lambda x, y: abs(x - y) < 1e-4 * 3000, foffset=lambda x, y: abs(x - y) < 0.5,
               bb_power=lambda x, y: abs(x / y - 1) < 2e-5, n0=lambda x, y: abs(x / y - 1) < 2e-4)
    for b in blocks:
        for key in keys:
            for got in (mine[b][1], sts[b]):
                assert bar[key](float(ref[b][1][key]), float(got[key])), (b, key, ref[b][1][key], got[key])


@pytest.mark.parametrize("flat", [False, True])
def test_reference_fm_c_runs_on_the_library(harness, flat):
    nb = 8
    iq = _signal("fm", 21, G0, nb)
    p = dict(FM, flat=int(flat))
    (ref, _), (mine, _), (auds, sts, filts) = _three(harness, "fm", iq, p, ["--flat"] if flat else [], G0, nb)
    # fm.c:121,130: the weak-sample threshold 0.55^2 avg_amp^2 is nowhere near a tie at this SNR
    for f in filts:
        t = np.abs(f.astype(np.complex128)) ** 2
        avg_amp = np.sqrt(t).sum() / (np.sqrt(2.0) * len(t))
        assert np.all(np.abs(t / (0.55 * 0.55 * avg_amp * avg_amp) - 1) > 0.01)
    assert all(len(a) == G0[1] // G0[3] for a, _ in ref)
    e_o, e_m = rel_rms(_cat(ref), np.concatenate(auds)), rel_rms(_cat(ref), _cat(mine))
    print("fm flat=%d: ref vs oracle %.3g, ref vs library thread %.3g" % (flat, e_o, e_m))
    assert e_o < 1e-5
    assert e_m < 1e-5
    _fm_bars(ref, mine, sts, range(1, nb))
    assert abs(ref[-1][1]["pdeviation"] - 3000) < 150


def test_reference_fm_squelch(harness):
    """fm.c:107-161: a carrier that drops for eight blocks.  The squelch closes one block after the SNR falls (the extra
    block flushes the filters), sends exact zeros, freezes foffset / pdeviation, and reopens."""
    nb, (fs, L_, _, D_) = 24, G0
    # seed: the noise-only estimate of fm.c:101-102 scatters around 0.83 over a block of 512 samples; this one keeps every
    # noise block below 0.86
    rng = np.random.default_rng(49)
    t = np.arange(nb * L_) / fs
    gate = np.ones(nb * L_)
    gate[8 * L_:16 * L_] = 0                                        # blocks 8..15: noise only, at the signal's noise level
    iq = (gate * 0.1 * np.exp(1j * (2 * np.pi * 20000.0 * t + 3.0 * np.sin(2 * np.pi * 1000 * t))) +
          1e-3 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))).astype(np.complex64)
    auds, sts, _ = _oracle(FM, iq, G0, nb)
    # the decision snr > 2 (fm.c:108-109) is not a tie: checked on the oracle before anything runs on the card.  The
    # pre-detection filter delays the signal by (M-1)/2 = half a block, so the edge blocks 8 and 16 are half signal, half
    # noise: their amplitude variance is large and their snr far below 1 like the noise blocks'
    snr = np.array([s["snr"] for s in sts])
    print("oracle snr per block:", np.array2string(snr, precision=3))
    # (block 0 is the start-up on an empty history, half zeros like an edge block: snr 0, squelch still open, fm.c:115)
    low = np.arange(1, nb)[snr[1:] <= 2]
    assert snr[0] < 1 and np.all(snr[low] < 1) and np.all(np.delete(snr, low)[1:] > 4)
    assert set(range(8, 16)) <= set(low.tolist()) <= set(range(8, 17))
    (ref, _), (mine, _), _ = _three(harness, "fm", iq, FM, [], G0, nb)
    zeros = [[b for b in range(nb) if not np.any(a[b])] for a in ([a for a, _ in ref], [a for a, _ in mine], auds)]
    print("blocks of exact zeros:", zeros[0])
    closed = [int(b) for b in low]
    # fm.c:112-115,155-161: the first low block still demodulates, the second sends zeros into the audio filter, whose
    # history (AM - 1 < AL samples) is all zeros from the third: exact zeros from there to the last low block
    assert zeros[0] == zeros[1] == zeros[2] == list(range(closed[0] + 2, closed[-1] + 1))
    last_open = closed[0] - 1
    for b in closed:                                                 # frozen, each side on its own last open block
        for key in ("foffset", "pdeviation"):
            assert ref[b][1][key] == ref[last_open][1][key]
            assert mine[b][1][key] == mine[last_open][1][key]
            assert sts[b][key] == sts[last_open][key]
    _fm_bars(ref, mine, sts, closed, ("foffset", "pdeviation"))     # ... and equal in all three
    reopen = closed[-1] + 1
    a_ref = _cat(ref, reopen + 2)
    assert rel_rms(a_ref, np.concatenate(auds[reopen + 2:])) < 1e-5
    assert rel_rms(a_ref, _cat(mine, reopen + 2)) < 1e-5


def test_reference_pl_tone(harness):
    """fm.c:189-285: pltask -- a decimate-by-32 slave of the audio master, a 16384-point real transform every 512 samples,
    peak bin.  The first run of the reference's fftwf_plan_dft_r2c_1d / fftwf_execute / window_rfilter calls on the
    library.  pltask races the hand-off, so plfreq is compared in the tail record only, written after the join."""
    nb, (fs, L_, _, _) = 24, G1
    rng = np.random.default_rng(23)
    t = np.arange(nb * L_) / fs
    ph = 2 * np.pi * 20000.0 * t + 3.0 * np.sin(2 * np.pi * 1000 * t) + 5.0 * np.sin(2 * np.pi * 100 * t)  # 3 kHz + 500 Hz deviation
    iq = (0.1 * np.exp(1j * ph) + 1e-3 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))).astype(np.complex64)
    (_, rtail), (_, mtail), (_, sts, _) = _three(harness, "fm", iq, FM, [], G1, nb)
    pl = [float(rtail[6]), float(mtail[6]), float(sts[-1]["plfreq"])]
    print("plfreq: reference's pltask %.4f, library thread %.4f, oracle %.4f" % tuple(pl))
    one_bin = 1500.0 / 16384                                          # 0.0916 Hz
    for x in pl:
        assert abs(x - 100.0) <= 1.0        # 1536 of 16384 samples: the main lobe's half-width is 1500 / 1536 Hz
    assert max(pl) - min(pl) <= one_bin * (1 + 1e-6)


# ---------------------------------------------------------------- linear (linear.c:21-322)
LINEAR_CASES = [("usb", dict(USB), ["--hang", "1.1", "--recovery", "6"], G0),
                ("isb", dict(USB, isb=1, channels=2), ["--hang", "1.1", "--recovery", "6", "--isb", "--stereo"], G0),
                ("shift", dict(USB, shift=300.0), ["--hang", "1.1", "--recovery", "6", "--shift", "300"], G0),
                ("usb-3840", dict(USB), ["--hang", "1.1", "--recovery", "6"], GEOMS[1]),
                ("usb-240k", dict(USB), ["--hang", "1.1", "--recovery", "6"], GEOMS[2])]


@pytest.mark.parametrize("name,p,extra,geom", LINEAR_CASES, ids=[c[0] for c in LINEAR_CASES])
def test_reference_linear_c_runs_on_the_library(harness, name, p, extra, geom):
    nb = 8
    iq = _signal("usb", 24, geom, nb)
    (ref, _), (mine, _), (auds, sts, _) = _three(harness, "linear", iq, p, extra, geom, nb)
    assert all(len(a) == p.get("channels", 1) * geom[1] // geom[3] for a, _ in ref)
    # the first block is the AGC start-up on numerically-zero samples (linear.c:271-272): compared from block 1 on
    e_o, e_m = rel_rms(_cat(ref, 1), np.concatenate(auds[1:])), rel_rms(_cat(ref, 1), _cat(mine, 1))
    print("linear %s: ref vs oracle %.3g, ref vs library thread %.3g" % (name, e_o, e_m))
    assert e_o < 1e-5
    assert e_m < 1e-5
    for b in range(1, nb):
        assert abs(ref[b][1]["gain"] / sts[b]["agc_gain"] - 1) < 2e-5, b
        assert abs(ref[b][1]["gain"] / mine[b][1]["gain"] - 1) < 2e-5, b
        assert abs(ref[b][1]["noise_gain"] / mine[b][1]["noise_gain"] - 1) < 1e-6, b   # set_filter under both threads


@pytest.mark.parametrize("mode", ["cam", "dsb"])
def test_reference_linear_pll(harness, mode):
    """linear.c:129-246 -- carrier search (the reference's fftwf_plan_dft_1d / fftwf_execute of 65536 points on the
    library), coarse + fine NCO, loop filter, lock hysteresis -- on the two signals and at the bars of
    test_gpu_parity.py::test_linear_carrier_pll.  The carrier offset sits on a bin centre of the search transform
    (k * 48000 / 65536 Hz), so the peak bin is not a tie."""
    nb, (fs, L_, _, _) = 64, G1
    binsize = 48000.0 / 65536
    t = np.arange(nb * L_) / fs
    rng = np.random.default_rng(41)
    msg = np.cos(2 * np.pi * 1000.0 * t)
    if mode == "cam":
        sig = 0.1 * (1 + 0.5 * msg) * np.exp(2j * np.pi * (20000.0 + 51 * binsize) * t)          # 37.35 Hz
        p = dict(demod="linear", low=-5000.0, high=5000.0, second_lo=-20000.0, hangtime=0.0, recovery_rate=50.0, pll=1)
        extra = ["--hang", "0", "--recovery", "50", "--pll"]
    else:
        sig = 0.1 * msg * np.exp(2j * np.pi * (20000.0 - 83 * binsize) * t + 0.7j)                # -60.79 Hz
        p = dict(demod="linear", low=-5000.0, high=5000.0, second_lo=-20000.0, hangtime=1.1, recovery_rate=6.0, pll=1, square=1)
        extra = ["--hang", "1.1", "--recovery", "6", "--pll", "--square"]
    iq = (sig + 1e-3 * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))).astype(np.complex64)
    (ref, _), (mine, _), (auds, sts, _) = _three(harness, "linear", iq, p, extra, G1, nb)
    for b in range(nb):
        r, m, o = ref[b][1], mine[b][1], sts[b]
        assert (int(r["pll_lock"]), int(r["lock_timer"])) == (int(m["pll_lock"]), int(m["lock_timer"])) == \
               (o["pll_lock"], o["lock_count"]), (b, r, m, o)
        for got_f, got_c in ((m["foffset"], m["cphase"]), (o["foffset"], o["cphase"])):
            np.testing.assert_allclose(r["foffset"], got_f, rtol=1e-3, atol=1e-3, err_msg="block %d" % b)
            np.testing.assert_allclose(r["cphase"], got_c, atol=2e-4, err_msg="block %d" % b)
    assert int(ref[-1][1]["pll_lock"]) == 1
    e_o, e_m = rel_rms(_cat(ref, 20), np.concatenate(auds[20:])), rel_rms(_cat(ref, 20), _cat(mine, 20))
    print("pll %s: ref vs oracle %.3g, ref vs library thread %.3g" % (mode, e_o, e_m))
    assert e_o < 2e-5
    assert e_m < 2e-5


# ---------------------------------------------------------------- packet (packet.c:201-212, 267-414)
FRAMES = [bytes([0x82, 0xA0, 0xA4, 0xA6, 0x40, 0x40, 0x60, 0x96, 0x82, 0x72, 0xA2, 0x40, 0x40, 0x61, 0x03, 0xF0]) +
          b"!4903.50N/07201.75W-test %d" % i for i in range(6)] + [bytes(range(1, 200)), bytes([0xFF] * 40)]
BLOCK = 1000
MAX_FRAME = 330                       # bytes, FCS included: packet.c:403 writes hdlc_frame[1024] without a bound
SESSIONS = [dict(amp=0.5, noise=0.0, ppm=0.0),        # clean
            dict(amp=0.3, noise=0.03, ppm=150.0),     # noisy
            dict(amp=0.4, noise=0.004, ppm=-450.0)]   # clock offset


def _packet_session(k, par):
    """Like _session_audio of test_gpu_packet.py: a short noise-only lead, good frames, and between them a frame with a
    flipped bit (bad FCS) and an aborted one (nine ones), as in test_bad_fcs_and_abort_are_dropped; then flags to the end."""
    rng = np.random.default_rng(300 + k)
    pick = [FRAMES[i] for i in rng.permutation(len(FRAMES))[:3]]
    if k == 0:
        pick[1] = FRAMES[6]                                          # a long one: 201 bytes with its FCS
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    bad = afsk_bits([FRAMES[(k + 3) % 6]], lead_flags=0, gap_flags=3)
    bad[8 * 8 + 50] ^= 1
    aborted = afsk_bits([FRAMES[(k + 4) % 6]], lead_flags=0, gap_flags=0)[:100] + [1] * 9 + flag * 4
    bits = (flag * (6 + k) + afsk_bits(pick[:1], lead_flags=0) + bad + afsk_bits(pick[1:2], lead_flags=0) + aborted +
            afsk_bits(pick[2:], lead_flags=0))
    assert all(len(f) + 2 <= MAX_FRAME for f in pick)
    return bits, pick


def _packet_input():
    """-> big-endian PCM [S, n_total], frames sent per session, datagram sizes"""
    built = [_packet_session(k, par) for k, par in enumerate(SESSIONS)]
    spb = 40.0 * (1 + 450e-6)
    n_total = int(max(len(b) for b, _ in built) * spb) + 4800 + 3 * BLOCK
    n_total -= n_total % BLOCK
    pcm = np.zeros((len(SESSIONS), n_total), ">i2")
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    for k, ((bits, _), par) in enumerate(zip(built, SESSIONS)):
        rng = np.random.default_rng(400 + k)
        bits = bits + flag * (n_total // 320 + 2)                     # every session idles on flags after its last frame
        x = afsk_audio(bits, amp=par["amp"], clock_ppm=par["ppm"])
        lead = 100 * k + 7                                           # noise-only lead, at most 0.1 s
        assert lead <= 4800
        y = (par["noise"] * rng.standard_normal(n_total)).astype(np.float32)
        y[lead:] += x[:n_total - lead]
        pcm[k] = np.round(np.clip(y, -0.999, 0.999) * 32767).astype(">i2")
    rng = np.random.default_rng(5)
    sizes, left = [333], n_total - 333                                # the first datagram of a session is short of a block
    while left:
        n = int(rng.choice([s for s in (1, 160, 333, 960, 1000) if s <= left]))
        sizes.append(n)
        left -= n
    return pcm, [[f + ax25_fcs(f) for f in pick] for _, pick in built], sizes


def _run_packet_driver(exe, libpath, pcm, sizes, timeout=CHILD_TIMEOUT):
    _run_packet_driver.last_rc = None
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            pos = 0
            for n in sizes:
                for k in range(pcm.shape[0]):
                    f.write(struct.pack("<II", 0x1000 + k, n) + pcm[k, pos:pos + n].tobytes())
                pos += n
        r = subprocess.run([exe, libpath, REF["packet"], fin, fout], capture_output=True, text=True, timeout=timeout)
        _run_packet_driver.last_rc = r.returncode
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
        blob = open(fout, "rb").read()
    posts, blocks, nses = struct.unpack_from("<qqq", blob, 0)
    pos, frames = 24, {}
    while pos < len(blob):
        ssrc, ln = struct.unpack_from("<II", blob, pos)
        frames.setdefault(ssrc - 0x1000, []).append(blob[pos + 8:pos + 8 + ln])
        pos += 8 + ln
    return posts, blocks, nses, frames


def test_reference_packet_c_runs_on_the_library(gpu):
    import ka9q_sdr_amd as kq
    from ka9q_sdr_amd import AfskBank
    _need("packet")
    pcm, sent, sizes = _packet_input()
    S, n_total = pcm.shape
    assert set(sizes) <= {1, 160, 333, 960, 1000} and sizes[0] < BLOCK and sum(sizes) == n_total
    # the oracle first: what it decodes, and that its frame_bit never nears the 8192 bits of packet.c's hdlc_frame[]
    oracles = [ko.Afsk() for _ in range(S)]
    for k in range(S):
        pos = 0
        for n in sizes:
            oracles[k].push_pcm_be(pcm[k, pos:pos + n].tobytes())
            pos += n
        assert oracles[k].max_frame_bit() < 8192 // 2, (k, oracles[k].max_frame_bit())
        assert oracles[k].frames() == sent[k], "session %d: the oracle decodes what was sent" % k
    # the bank, same chunking
    bank = AfskBank(S, max_frames=16)
    pos = 0
    for n in sizes:
        bank.push_pcm_be(pcm[:, pos:pos + n])
        pos += n
    got_bank = [bank.frames(k) for k in range(S)]
    counts = [bank.state(k)["decoded_packets"] for k in range(S)]
    assert all(bank.dropped(k) == 0 for k in range(S))
    bank.close()
    # the reference's main loop and decode_task on the library
    exe = os.path.join(tempfile.gettempdir(), "kq_packet_driver_%d" % os.getpid())
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-Wall", os.path.join(ROOT, "tests", "dropin", "packet_driver.c"),
                        "-ldl", "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    try:
        posts, blocks, nses, got_ref = _guard("reference packet.c", _run_packet_driver, exe, kq.library_path(), pcm, sizes)
    finally:
        os.unlink(exe)
    assert (blocks, nses) == (S * (n_total // BLOCK), S)
    assert posts == blocks + S, "a decoder thread skipped a block (%d posts for %d blocks of %d sessions)" % (posts, blocks, S)
    for k in range(S):
        assert got_ref.get(k, []) == got_bank[k] == oracles[k].frames(), "session %d" % k
        assert got_ref.get(k, []) == sent[k], "session %d decodes what was sent" % k
        assert counts[k] == len(got_ref.get(k, [])), k
