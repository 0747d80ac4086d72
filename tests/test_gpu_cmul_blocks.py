"""The block forms of the complex products (rfft::pk_cmul2 / pk_cmul4 and kin, kq_regfft.hpp) in every kernel body that
uses them: the 16384-point full-spectrum kernel's three mixes (PLAIN 1, 0 and 2), pass 1's and pass 2's twiddles, and the
N = 65536 mixes (BIG 1 and 2); beside them the pruned kernel, which shares the header's single products and butterflies.

The kernels' N is fixed, so the shapes are small in channels and blocks: 3 channels (1 at N = 65536), 2 calls of 2 blocks,
so that the history and the oscillator carry from call to call matter.  The unswept cases hold one channel on an LO that
is a whole number of bins: its row phasors are exactly 1.

Filter output, audio, n0 and the status fields are held against the oracle by test_gpu_parity._compare, at its tolerances.
For the N = 16384 cases one channel's master spectrum is pulled (kq_bank_pull_spectrum) and held against float64
arithmetic both ways the existing spectrum tests do: compute_n0 on it (common.n0_float64, test_gpu_parity's 2e-5) and its
float64 inverse transform against the mixed samples (test_gpu_golden's 2e-6 of the amplitude).
"""
import functools

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd import workload as wl
import kq_oracle as ko
from common import bank_cfg, n0_float64, oracle_cfg
from test_gpu_full16k_tables import _dyadic, _fm
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

PER, NCALLS = 2, 2
NBLOCKS = PER * NCALLS
GEOM16 = dict(samprate=10000000, L=8192, M=8193, D=256)                     # cfg 4's geometry: N = 16384, N/D = 64
GEOM64 = {k: wl.GEOMETRY["cfg5"][k] for k in ("samprate", "L", "M", "D")}   # N = 65536
SPEC_CH = 1          # the channel whose spectrum is pulled: fractional LO; the one the retune case retunes
SWEEP16 = 2000.0     # Hz/s: 2e-11 cycles per sample^2 at 10 MS/s, inside kSweepLimit16k = 4.8e-11 (kq_full16k.hip)
SWEEP64_LIMIT = 1.1e-11   # kSweepLimit64k


def _plan16(case):
    fs = GEOM16["samprate"]
    assert (wl.emitter_freq(24, fs) * 16384 / fs) % 1 == 0
    plan = [_fm(fs, 24, 0.0), _fm(fs, 25, 777.7), _fm(fs, 40, -1.3)]   # bin-aligned, fractional, negative
    if case == "swept":
        for c, p in enumerate(plan):      # every channel of the launch sweeps: the swept steady-state variant
            p.update(doppler=_dyadic(300.0 * (c + 1), fs), doppler_rate=SWEEP16 * (1 if c % 2 else -1) / (c + 1))
            assert 0 < abs(p["doppler_rate"]) / fs ** 2 < 4.8e-11
    return plan


def _plan64(case):
    fs = GEOM64["samprate"]
    plan = wl.channel_plan("cfg5", 1, first=4)        # emitter 19: bin -11520 of 65536
    p = plan[0]
    assert 0 < abs(p["doppler_rate"]) / fs ** 2 < SWEEP64_LIMIT
    if case == "unswept64":
        p["second_lo"] -= p["doppler"]
        p["doppler"] = p["doppler_rate"] = 0.0
        assert (p["second_lo"] * 65536 / fs) % 1 == 0
    return plan


def _case(case):
    """-> (geometry, plan, compute_n0, forward mode, {block: (channel, new second LO)})"""
    if case in ("swept64", "unswept64"):
        return GEOM64, _plan64(case), True, kq.KQ_FWD_FULL, {}
    plan = _plan16(case)
    ev = {PER: (SPEC_CH, _dyadic(plan[SPEC_CH]["second_lo"] + 4321.0, GEOM16["samprate"]))} if case == "retune" else {}
    return GEOM16, plan, case != "pruned", kq.KQ_FWD_PRUNED if case == "pruned" else kq.KQ_FWD_FULL, ev


@functools.lru_cache(maxsize=None)
def _iq(big):
    g = GEOM64 if big else GEOM16
    iq = wl.make_iq(g["samprate"], NBLOCKS * g["L"], seed=47).astype(np.complex64)
    iq.setflags(write=False)
    return iq


def _oracle(case):
    g, plan, n0, _, ev = _case(case)
    fs, L, M = g["samprate"], g["L"], g["M"]
    iq = _iq(g is GEOM64)
    chans = [ko.Channel(oracle_cfg(p, fs, L, M, g["D"], compute_n0=int(n0))) for p in plan]
    want = [([], [], []) for _ in plan]
    for b in range(NBLOCKS):
        if b in ev:
            chans[ev[b][0]].set_lo2(ev[b][1])
        for c, ch in enumerate(chans):
            a, st, f, _ = ch.block(iq[b * L:(b + 1) * L], want_filt=True)
            want[c][0].append(a)
            want[c][1].append(st)
            want[c][2].append(f)
    for ch in chans:
        ch.close()
    return want


def _bank(case, spectrum=False):
    """the case on the bank -> per channel dict(audio, status, filt) as test_gpu_parity._run_bank, and SPEC_CH's spectra"""
    g, plan, n0, mode, ev = _case(case)
    L = g["L"]
    iq = _iq(g is GEOM64)
    bank = kq.Bank(g["samprate"], L, g["M"], g["D"], len(plan), PER, compute_n0=n0, fwd_mode=mode)
    for p in plan:
        bank.add_channel(bank_cfg(p))
    if spectrum:
        bank.arm_spectrum(SPEC_CH)
    res = [dict(audio=[], status=[], filt=[]) for _ in plan]
    spectra = []
    for b0 in range(0, NBLOCKS, PER):
        if b0 in ev:
            bank.set_second_lo(*ev[b0])
        bank.push_iq(iq[b0 * L:(b0 + PER) * L])
        assert bank.process() == PER
        for c in range(len(plan)):
            for k in range(PER):
                res[c]["audio"].append(bank.audio(c, k))
                res[c]["status"].append(bank.status(c, k))
                res[c]["filt"].append(bank.filter_output(c, k))
        if spectrum:
            spectra += [bank.spectrum(SPEC_CH, k) for k in range(PER)]
    assert bank.fwd_mode == mode
    bank.close()
    return res, spectra


@pytest.mark.parametrize("case", ["steady", "retune", "swept", "pruned", "unswept64", "swept64"])
def test_against_the_oracle(gpu, case):
    g, plan, n0, _, _ = _case(case)
    got, _ = _bank(case)
    _compare(plan, got, _oracle(case), check_n0=n0, geom=g)


def _phase_turns(case, n):
    """SPEC_CH's oscillator phase in turns at sample n (counted from the first sample pushed), float64: second LO, minus the
    Doppler oscillator (set_doppler mixes with exp(-j 2 pi d t)), carried over the retune"""
    g, plan, _, _, ev = _case(case)
    fs = g["samprate"]
    p = plan[SPEC_CH]
    f = p["second_lo"] / fs
    ph = f * n
    for b, (c, hz) in ev.items():
        assert c == SPEC_CH
        n0 = b * g["L"]
        ph = np.where(n < n0, ph, f * n0 + hz / fs * (n - n0))
    d, r = p.get("doppler", 0.0) / fs, p.get("doppler_rate", 0.0) / fs ** 2
    return ph - (d * n + r * 0.5 * n * (n - 1.0))


@pytest.mark.parametrize("case", ["steady", "retune", "swept"])
def test_master_spectrum_against_float64(gpu, case):
    g, plan, _, _, _ = _case(case)
    fs, L, M = g["samprate"], g["L"], g["M"]
    got, spectra = _bank(case, spectrum=True)
    assert len(spectra) == NBLOCKS
    p = plan[SPEC_CH]
    x = np.concatenate([np.zeros(M - 1, np.complex64), _iq(False)]).astype(np.complex128)
    n0 = None
    for b, spec in enumerate(spectra):
        # compute_n0 in float64 on the kernel's own spectrum, smoothed as fm.c:82 does (test_gpu_parity._n0_ties_are_ties)
        fresh = n0_float64(spec, fs, p["low"], p["high"])
        n0 = fresh if n0 is None else n0 + 0.01 * (fresh - n0)
        print("block %d: n0 %.8g / float64 %.8g" % (b, got[SPEC_CH]["status"][b]["n0"], n0), end="")
        np.testing.assert_allclose(got[SPEC_CH]["status"][b]["n0"], n0, rtol=2e-5, err_msg="block %d" % b)
        # the window's mixed samples back from the spectrum in float64 (test_gpu_golden._mixed_samples)
        n = np.arange(b * L - (M - 1), (b + 1) * L, dtype=np.float64)
        want = x[b * L:b * L + L + M - 1] * np.exp(2j * np.pi * _phase_turns(case, n))
        err = np.abs(np.fft.ifft(spec.astype(np.complex128)) - want).max() / np.abs(want).max()
        print("  mixed samples: %.3g of the largest" % err)
        assert err < 2e-6, (case, b, err)
