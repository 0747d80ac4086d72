"""The default step's two kernels after their non-arithmetic instructions were thinned out: results unchanged.

Filter (k_filter_full16k, N = 16384, N/D = 64, compute_n0 on).  The tail of the kernel -- the slave's bins into LDS, the
epilogue's prefetch, compute_n0's reductions -- keeps wave-uniform quantities on the scalar unit and leaves the prefetch
registers of the seven waves that run no epilogue undefined.  Held against the oracle with the tolerances of
tests/test_gpu_parity.py, on a mix of channels that takes every branch of that tail: de-emphasised and flat FM, a linear
channel without ISB, one with ISB (the second response bin of the prefetch) and a linear channel whose passband straddles
bin 0 (bins on both sides of the spectrum's seam go to the slave), three blocks per call (an odd count).  The channels of a
bank share one I/Q stream, so "a channel fed zeros" is the same bank on a stream of zeros: every spectrum is then all zero
and compute_n0 leaves its packed fast path for the loop that spells the reference's comparisons out.
The steady-state instance (PLAIN == 1) and the general one (which redoes the first block of a retuned channel) share that
tail: a twin bank whose channel 1 is retuned to its own frequency just before the second call must agree bit for bit in
what the filter kernel writes -- the filter output and compute_n0's figure, the planes tests/test_gpu_full16k_tables.py
holds a twin to.

Demodulator (k_demod64, N/D = 64).  The four-wave pipeline and the one-wave form compute "every value by the same
expressions"; the launch takes the one-wave form above 2048 workgroups.  Channels 0-2 of a 3-channel and of a
2052-channel bank, configured alike and fed alike, must agree in every audio sample and every status field (compute_n0 on: the n0
chain included), over ten blocks in calls of one, two and five (an odd count: the last pair of a call is half empty).
"""
import functools

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd import workload as wl
import kq_oracle as ko
from common import bank_cfg, oracle_cfg, rel_rms

pytestmark = pytest.mark.gpu

FILT_TOL = 1e-5            # as tests/test_gpu_parity.py: relative RMS against the oracle
AUDIO_TOL = 1e-5
FIRST_LINEAR_TOL = 4e-3    # a linear channel's first block: AGC start-up on numerically-zero samples (test_gpu_parity.py)
N0_RTOL = 2e-4

GEOM = dict(samprate=10000000, L=8192, M=8193, D=256)      # cfg 4's geometry: the headline instance (EPI = 1)
PER, NCALLS = 3, 2


def _dyadic(hz, fs):
    """hz moved onto a multiple of fs / 2^20: the host's closed-form phases are then exact in double whatever sample they
    are referred to, so the twin, which re-references channel 1's oscillator at the retune, stages the same bits
    (tests/test_gpu_full16k_tables.py)."""
    return round(hz / fs * 2 ** 20) / 2 ** 20 * fs


def _filter_plan():
    fs = GEOM["samprate"]
    f = lambda e, off: _dyadic(-wl.emitter_freq(e, fs) + off, fs)
    return [dict(demod="fm", low=-8000.0, high=8000.0, second_lo=f(24, 0.0)),                    # de-emphasised, bin-aligned LO
            dict(demod="fm", low=-8000.0, high=8000.0, second_lo=f(25, 777.7), flat=1),           # flat, fractional LO
            dict(demod="linear", low=100.0, high=3000.0, second_lo=f(27, 0.0), hangtime=1.1, recovery_rate=6.0),
            dict(demod="linear", low=-5000.0, high=5000.0, second_lo=f(31, -1.3), hangtime=1.1, recovery_rate=6.0),
            dict(demod="linear", low=-5000.0, high=5000.0, second_lo=f(35, 12.5), isb=1, channels=2, hangtime=1.1,
                 recovery_rate=6.0)]


@functools.lru_cache(maxsize=None)
def _iq(zeros):
    n = PER * NCALLS * GEOM["L"]
    iq = np.zeros(n, np.complex64) if zeros else wl.make_iq(GEOM["samprate"], n, seed=43)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def _oracle(zeros):
    """per channel: [(filt, audio, status)] block by block, computed once"""
    fs, L = GEOM["samprate"], GEOM["L"]
    iq = _iq(zeros)
    out = []
    for p in _filter_plan():
        ch = ko.Channel(oracle_cfg(p, fs, L, GEOM["M"], GEOM["D"], compute_n0=1))
        rows = []
        for b in range(PER * NCALLS):
            a, st, f, _ = ch.block(iq[b * L:(b + 1) * L], want_filt=True)
            rows.append((f, a, st))
        ch.close()
        out.append(rows)
    return out


def _bank_run(zeros, retune=None):
    """-> per channel: [(filt, audio, status)]; `retune`: the channel set to its own frequency before the second call"""
    fs, L = GEOM["samprate"], GEOM["L"]
    iq = _iq(zeros)
    plan = _filter_plan()
    bank = kq.Bank(fs, L, GEOM["M"], GEOM["D"], len(plan), PER, compute_n0=True, fwd_mode=kq.KQ_FWD_FULL)
    for p in plan:
        bank.add_channel(bank_cfg(p))
    out = [[] for _ in plan]
    for call in range(NCALLS):
        if call == 1 and retune is not None:
            bank.set_second_lo(retune, plan[retune]["second_lo"])
        bank.push_iq(iq[call * PER * L:(call + 1) * PER * L])
        assert bank.process() == PER
        for c in range(len(plan)):
            for k in range(PER):
                out[c].append((bank.filter_output(c, k), bank.audio(c, k), bank.status(c, k)))
    assert bank.fwd_mode == kq.KQ_FWD_FULL
    bank.close()
    return out


def test_filter_tail_against_oracle_and_retuned_twin(gpu):
    plan = _filter_plan()
    got, want = _bank_run(False), _oracle(False)
    for c, p in enumerate(plan):
        for b in range(PER * NCALLS):
            (fg, ag, sg), (fw, aw, sw) = got[c][b], want[c][b]
            ef = rel_rms(fg, fw)
            assert len(ag) == len(aw), (c, b)
            ea = rel_rms(ag, aw)
            print("channel %d (%s) block %d: filter %.3g  audio %.3g  n0 %.6g / %.6g" % (c, p["demod"], b, ef, ea, sg["n0"], sw["n0"]))
            assert ef < FILT_TOL, ("filter", c, b, ef)
            first_linear = p["demod"] == "linear" and b == 0
            assert ea < (FIRST_LINEAR_TOL if first_linear else AUDIO_TOL), ("audio", c, b, ea)
            np.testing.assert_allclose(sg["n0"], sw["n0"], rtol=N0_RTOL, err_msg="n0 (%d, %d)" % (c, b))
    twin = _bank_run(False, retune=1)
    for c in range(len(plan)):
        for b in range(PER * NCALLS):
            assert np.array_equal(got[c][b][0], twin[c][b][0]), ("filter output differs from the retuned twin", c, b)
            assert got[c][b][2]["n0"] == twin[c][b][2]["n0"], ("n0 differs from the retuned twin", c, b)
    # channel 1's first block of the second call went through the general instance, every other channel-block through the
    # steady-state one on both banks: the audio and the status records behind them are the same arithmetic on the same bits
    for c in range(len(plan)):
        for b in range(PER * NCALLS):
            assert np.array_equal(got[c][b][1], twin[c][b][1]), ("audio differs from the retuned twin", c, b)
            assert _same_status(got[c][b][2], twin[c][b][2]), ("status", c, b, got[c][b][2], twin[c][b][2])


def _same_status(a, b):
    assert a.keys() == b.keys()
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def test_filter_tail_on_zeros_takes_the_slow_path_of_compute_n0(gpu):
    plan = _filter_plan()
    got, want = _bank_run(True), _oracle(True)
    twin = _bank_run(True, retune=1)
    for c in range(len(plan)):
        for b in range(PER * NCALLS):
            (fg, _, sg), (fw, _, sw) = got[c][b], want[c][b]
            assert not np.any(fw) and not np.any(fg), ("filter output of a zero stream", c, b)
            print("channel %d block %d: n0 %r / %r" % (c, b, sg["n0"], sw["n0"]))
            np.testing.assert_allclose(sg["n0"], sw["n0"], rtol=N0_RTOL, err_msg="n0 (%d, %d)" % (c, b))
            assert np.array_equal(fg, twin[c][b][0])
            assert np.array_equal(np.float32(sg["n0"]), np.float32(twin[c][b][2]["n0"]), equal_nan=True), (c, b)


# ---------------------------------------------------------------- demodulator: four waves against one

DGEOM = dict(samprate=768000, L=512, M=513, D=16)     # N = 1024, N/D = 64, 32 samples per block at 48 kHz
DTOTAL = 10                                           # blocks in all, whatever the call length


def _demod_plan(nchan):
    fs = DGEOM["samprate"]
    on = -wl.emitter_freq(24, fs)
    plan = [dict(demod="fm", low=-8000.0, high=8000.0, second_lo=on),                 # de-emphasised, strong carrier
            dict(demod="fm", low=-8000.0, high=8000.0, second_lo=on + 150000.0),      # de-emphasised, noise only: the squelch closes
            dict(demod="fm", low=-8000.0, high=8000.0, second_lo=on + 2.5, flat=1)]   # flat (one wave in either launch)
    for k in range(3, nchan):
        plan.append(dict(demod="fm", low=-8000.0, high=8000.0, second_lo=on + 37.0 * (k % 97) - 1500.0, flat=k % 2))
    return plan


def _demod_run(nchan, dblocks):
    """-> per channel 0-2: [(audio, status)] of the DTOTAL blocks, taken `dblocks` per call; compute_n0 on, so that the n0
    chain through the blocks is part of every record"""
    fs, L = DGEOM["samprate"], DGEOM["L"]
    iq = wl.make_iq(fs, DTOTAL * L, seed=47, emitters=[24])
    bank = kq.Bank(fs, L, DGEOM["M"], DGEOM["D"], nchan, dblocks, compute_n0=True)
    got = bank.add_channels([bank_cfg(p) for p in _demod_plan(nchan)])
    assert list(got) == list(range(nchan))
    out = [[] for _ in range(3)]
    for call in range(DTOTAL // dblocks):
        bank.push_iq(iq[call * dblocks * L:(call + 1) * dblocks * L])
        assert bank.process() == dblocks
        for c in range(3):
            out[c] += [(bank.audio(c, k), bank.status(c, k)) for k in range(dblocks)]
    bank.close()
    return out


@pytest.mark.parametrize("dblocks", [1, 2, 5])
def test_demod64_four_waves_and_one_wave_agree_bit_for_bit(gpu, dblocks):
    """Before the de-emphasis filter's complex products had their rounding steps spelled out (cmul_as in kq_demod64.hip) the
    two forms were one set of expressions in the source and two sets of rounding steps as compiled: 152 and 142 of the 320
    audio samples of channels 0 and 1 differed, by up to 2.98e-08 (profiles/r09/demod_forms.txt).  Since then both forms call
    one set of stage functions.  Blocks per call: 1, a lone half pair (the pipeline fills and drains without a block b+1);
    2, one full pair; 5, two pairs and a half one.  Ten blocks in all either way."""
    small, big = _demod_run(3, dblocks), _demod_run(2052, dblocks)      # 3 workgroups: four waves per de-emphasised channel; 2052: one wave
    closed = False
    for c in range(3):
        for k in range(DTOTAL):
            (a4, s4), (a1, s1) = small[c][k], big[c][k]
            assert len(a4) == 32
            assert np.array_equal(a4, a1), ("audio", c, k)
            assert _same_status(s4, s1), ("status", c, k, s4, s1)
            assert not np.isnan(s4["n0"]), ("n0", c, k)
            closed |= c == 1 and s4["squelch_count"] >= 2
    for k in range(4, DTOTAL):      # (from the block on at which the five-blocks-per-call form of this test looked)
        assert small[0][k][1]["squelch_count"] == 0, "the carrier's channel stays open"
    assert closed, "the noise-only channel's squelch closes"
    assert np.any(small[0][4][0]) and np.any(small[2][4][0])
