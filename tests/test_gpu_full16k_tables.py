"""The 16384-point full-spectrum kernel's row-phasor plane (ChanDev::row_ph), with compute_n0 on.

The steady-state variant of the kernel takes the 32 row phasors of a channel from a per-channel plane that the host
rebuilds when a channel's frequency step changes.  These tests walk the plane through every event that changes a step
-- retune, a channel leaving and another joining in its slot, a sweep switched on and off again -- and hold every
channel-block against the oracle; a twin bank fed one block per call must agree bit for bit in what the filter kernel
writes (the same block is then the first of its call, where a retuned channel goes through the variant that evaluates
the table in the kernel).
compute_n0 is on throughout: it runs in the same kernel, on the bins the mix feeds.

N = 16384 (L = 8192, M = 8193); N/D = 64 (the one-wave epilogue) and N/D = 256 (the R-wave epilogue).
"""
import functools

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd import workload as wl
import kq_oracle as ko
from common import bank_cfg, oracle_cfg, rel_rms

pytestmark = pytest.mark.gpu

FILT_TOL = 1e-5     # as tests/test_gpu_parity.py: relative RMS against the oracle
AUDIO_TOL = 1e-5
N0_RTOL = 2e-4

GEOMS = {"nd64": dict(samprate=10000000, L=8192, M=8193, D=256),     # cfg 4's geometry: EPI = 1
         "nd256": dict(samprate=2000000, L=8192, M=8193, D=64)}      # cfg 2's geometry: EPI = 2
PER, NCALLS = 2, 5
NBLOCKS = PER * NCALLS
SWEEP = (1500.0, 80.0)    # Hz, Hz/s: 2e-11 cycles/sample^2 at 2 MS/s, inside the steady-state variant's 4.8e-11


def _dyadic(hz, fs):
    """hz moved (by less than fs / 2^21) onto a multiple of fs / 2^20.  Bins are fs / 2^14 apart, so such a frequency is
    still as fractional as any; but the host's closed-form phases phase + step * k are then exact in double whatever sample
    they are referred to -- and the two banks of the twin comparison, which re-reference their oscillators at different
    samples (after every non-steady call, and a channel at a time in the steady state), stage the same bits."""
    return round(hz / fs * 2 ** 20) / 2 ** 20 * fs


def _fm(fs, e, off):
    p = wl._mode_params("fm", e)
    p.update(second_lo=_dyadic(-wl.emitter_freq(e, fs) + off, fs), doppler=0.0, doppler_rate=0.0)
    return p


def _plan(fs):
    """slot (relative) -> channel: 0 on a bin-aligned LO (emitter 24 sits on bin -1728 of 16384), 1 fractional, 2 left
    empty, 3 negative; `join` takes slot 1 over half way."""
    assert (wl.emitter_freq(24, fs) * 16384 / fs) % 1 == 0
    return {0: _fm(fs, 24, 0.0), 1: _fm(fs, 25, 777.7), 3: _fm(fs, 40, -1.3)}, _fm(fs, 28, 12.5)


@functools.lru_cache(maxsize=None)
def _iq(name):
    g = GEOMS[name]
    iq = wl.make_iq(g["samprate"], NBLOCKS * g["L"], seed=41)
    iq.setflags(write=False)
    return iq


def _events(fs):
    """block index at which the event takes effect -> what it does to (set_lo, set_doppler, replace)"""
    plan, join = _plan(fs)
    return {2: ("lo", 0, _dyadic(plan[0]["second_lo"] + 777.7, fs)),     # between calls 1 and 2: a retune
            4: ("replace", 1, join),                        # between calls 2 and 3: slot 1 changes hands
            6: ("doppler", 3, SWEEP),                       # between calls 3 and 4: a sweep inside the limit
            8: ("doppler", 3, (0.0, 0.0))}                  # and back to zero for call 5


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """{(slot, block): (filt, audio, n0)} of the sequence, computed once per geometry"""
    g = GEOMS[name]
    fs, L, M = g["samprate"], g["L"], g["M"]
    iq = _iq(name)
    plan, _ = _plan(fs)
    ev = _events(fs)
    chans = {s: ko.Channel(oracle_cfg(p, fs, L, M, g["D"], compute_n0=1)) for s, p in plan.items()}
    out = {}
    for b in range(NBLOCKS):
        if b in ev:
            kind, s, arg = ev[b]
            if kind == "lo":
                chans[s].set_lo2(arg)
            elif kind == "doppler":
                chans[s].set_doppler(*arg)
            else:
                chans[s].close()
                chans[s] = ko.Channel(oracle_cfg(arg, fs, L, M, g["D"], compute_n0=1))
                chans[s].prime_history(iq[b * L - (M - 1):b * L])
        for s, ch in chans.items():
            a, st, f, _ = ch.block(iq[b * L:(b + 1) * L], want_filt=True)
            out[(s, b)] = (f, a, st["n0"])
    for ch in chans.values():
        ch.close()
    return out


def _bank_sequence(name, per, fill):
    """The sequence on a bank fed `per` blocks per call, its four slots behind `fill` other channels (and two more behind
    them when there are any, so that the slots are in the middle of the bank); -> {(slot, block): (filt, audio, n0)}"""
    g = GEOMS[name]
    fs, L = g["samprate"], g["L"]
    iq = _iq(name)
    plan, _ = _plan(fs)
    ev = _events(fs)
    tail = 2 if fill else 0
    bank = kq.Bank(fs, L, g["M"], g["D"], 96 if fill else 4, per, compute_n0=True, fwd_mode=kq.KQ_FWD_FULL)
    filler = [_fm(fs, (20, 21, 32, 33)[k % 4], 2.5 + k) for k in range(fill)]
    mine = [plan[0], plan[1], _fm(fs, 29, 0.0), plan[3]]                    # (slot 2 is emptied below)
    got = bank.add_channels([bank_cfg(p) for p in filler + mine + filler[:tail]])
    assert list(got) == list(range(fill + 4 + tail))
    bank.remove_channel(fill + 2)                                           # the empty slot: launches go over a channel list
    assert not bank.channel_active(fill + 2)
    out = {}
    for b0 in range(0, NBLOCKS, per):
        for b in range(b0, b0 + per):
            if b not in ev:
                continue
            assert b == b0, "events fall on call boundaries"
            kind, s, arg = ev[b]
            if kind == "lo":
                bank.set_second_lo(fill + s, arg)
            elif kind == "doppler":
                bank.set_doppler(fill + s, *arg)
            else:
                bank.remove_channel(fill + s)
                assert bank.add_channel(bank_cfg(arg)) == fill + s          # the lowest hole: the same slot
        bank.push_iq(iq[b0 * L:(b0 + per) * L])
        assert bank.process() == per
        for s in plan:
            for k in range(per):
                out[(s, b0 + k)] = (bank.filter_output(fill + s, k), bank.audio(fill + s, k), bank.status(fill + s, k)["n0"])
    assert bank.fwd_mode == kq.KQ_FWD_FULL
    bank.close()
    return out


def _against_oracle(got, want):
    assert got.keys() == want.keys()
    for key in sorted(want):
        (fg, ag, ng), (fw, aw, nw) = got[key], want[key]
        ef = rel_rms(fg, fw)
        print("slot %d block %d: filter %.3g" % (key[0], key[1], ef), end="")
        assert ef < FILT_TOL, ("filter", key, ef)
        assert len(ag) == len(aw), ("audio length", key)
        ea = rel_rms(ag, aw)
        print("  audio %.3g  n0 %.6g / %.6g" % (ea, ng, nw))
        assert ea < AUDIO_TOL, ("audio", key, ea)
        np.testing.assert_allclose(ng, nw, rtol=N0_RTOL, err_msg="n0 %s" % (key,))


def _bit_for_bit(a, b):
    """What the filter kernel writes -- the filter output and compute_n0's figure -- bit for bit.  (Not the audio: the fused
    FM demodulator takes a call's blocks in pairs, two to a wave, so its own sums run in another order in a call of one
    block than in a call of two; the twin's audio is held against the oracle instead, by the caller.)"""
    assert a.keys() == b.keys()
    same_audio = 0
    for key in sorted(a):
        assert np.array_equal(a[key][0], b[key][0]), ("filter output differs from the one-block-per-call twin", key)
        assert a[key][2] == b[key][2], ("n0 differs from the one-block-per-call twin", key, a[key][2], b[key][2])
        same_audio += bool(np.array_equal(a[key][1], b[key][1]))
    print("twin: filter output and n0 identical in %d channel-blocks; audio identical in %d of them" % (len(a), same_audio))


@pytest.mark.parametrize("name", ["nd64", "nd256"])
def test_sequence_matches_oracle_and_twin(gpu, name):
    """Retune, slot handed over, sweep on, sweep off: every channel-block against the oracle, and bit for bit against a
    twin bank fed one block per call."""
    got = _bank_sequence(name, PER, 0)
    _against_oracle(got, _oracle(name))
    twin = _bank_sequence(name, 1, 0)
    _bit_for_bit(got, twin)
    _against_oracle(twin, _oracle(name))


@pytest.mark.parametrize("name", ["nd64", "nd256"])
def test_sequence_at_channel_numbers_from_64_on(gpu, name):
    """The same sequence in slots 64..67 of a bank created for 96 channels, with channels in front and behind and a hole
    among them (launches over a channel list): the plane is indexed by slot, not by rank in the list."""
    got = _bank_sequence(name, PER, 64)
    _against_oracle(got, _oracle(name))
    twin = _bank_sequence(name, 1, 64)
    _bit_for_bit(got, twin)
    _against_oracle(twin, _oracle(name))


@pytest.mark.parametrize("per,ncalls", [(1, 8), (2, 4)])
def test_every_channel_retuned_before_every_call(gpu, per, ncalls):
    """A host that retunes every channel before every call: a row left over from the call before would mix the blocks
    behind the first of a call (and, one block per call, nothing: every block is then redone by the general variant --
    the issue's case, kept as the cross-check) with the wrong oscillator."""
    g = GEOMS["nd64"]
    fs, L, M = g["samprate"], g["L"], g["M"]
    iq = _iq("nd64")
    plan, _ = _plan(fs)
    slots = sorted(plan)
    chans = {s: ko.Channel(oracle_cfg(plan[s], fs, L, M, g["D"], compute_n0=1)) for s in slots}
    bank = kq.Bank(fs, L, M, g["D"], len(slots), per, compute_n0=True, fwd_mode=kq.KQ_FWD_FULL)
    for s in slots:
        bank.add_channel(bank_cfg(plan[s]))
    for call in range(ncalls):
        for c, s in enumerate(slots):
            hz = plan[s]["second_lo"] + (12.5 + 3.1 * c) * (call + 1)
            bank.set_second_lo(c, hz)
            chans[s].set_lo2(hz)
        bank.push_iq(iq[per * call * L:per * (call + 1) * L])
        assert bank.process() == per
        for c, s in enumerate(slots):
            for k in range(per):
                b = per * call + k
                _, st, filt, _ = chans[s].block(iq[b * L:(b + 1) * L], want_filt=True)
                e = rel_rms(bank.filter_output(c, k), filt)
                n0 = bank.status(c, k)["n0"]
                print("call %d channel %d block %d: filter %.3g  n0 %.6g / %.6g" % (call, c, k, e, n0, st["n0"]))
                assert e < FILT_TOL, (call, c, k, e)
                np.testing.assert_allclose(n0, st["n0"], rtol=N0_RTOL, err_msg="n0 (%d, %d, %d)" % (call, c, k))
    bank.close()
    for ch in chans.values():
        ch.close()
