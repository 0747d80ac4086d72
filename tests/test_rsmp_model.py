"""The resampler's definition (include/ka9q_hip.h, kq_rsmp_*) on the CPU, through the float64 model of tests/rsmp_model.py:
the count of outputs per call, the filter's gain in its passband and stopband, and what it is for -- AFSK-1200 audio at a
receiver's 50 000, 39 062.5 and 31 250 Hz, which packet.c's decoder (the oracle's Afsk) cannot read as it is and reads
after resampling to 48 kHz; the last of these through the oracle's whole receive chain, as the GPU test runs it."""
import functools

import numpy as np
import pytest

import kq_oracle as ko
import rsmp_model as rm
from common import afsk_audio, afsk_bits, ax25_fcs, run_oracle

SPLITS = (1, 1, 7, 100, 1, 3)


@pytest.mark.parametrize("P,Q", [(24, 25), (768, 625), (1, 4), (3, 2), (1, 16), (16, 1), (147, 160)])
def test_outputs_per_call(P, Q):
    """J = ceil((n0 + S) P / Q) - ceil(n0 P / Q) counts the j with n0 <= floor(j Q / P) < n0 + S, and the calls of a split
    stream add up to the unsplit count"""
    for n0 in (0, 1, 5, 24, 25, 26, 1000, 17 << 28):
        for S in (0, 1, 2, 7, 100, 625):
            j_lo = max(0, n0 * P // Q - 2)
            brute = sum(1 for j in range(j_lo, (n0 + S) * P // Q + 3) if n0 <= j * Q // P < n0 + S)
            assert rm.count(n0, S, P, Q) == brute, (n0, S)
    n, total = 0, 0
    for S in SPLITS:
        total += rm.count(n, S, P, Q)
        n += S
    assert total == rm.count(0, n, P, Q) == rm.ceil_div(n * P, Q)


# in_rate_num, in_rate_den, T, beta
TONES = [(50000, 1, 32, 3.0), (10000000, 256, 32, 3.0), (192000, 1, 96, 3.0)]


@pytest.mark.parametrize("num,den,T,beta", TONES)
def test_tone_gains(num, den, T, beta):
    """with the clean cutoff a 1 kHz tone comes through within 0.1 dB, and a tone 500 Hz above the stopband edge (cutoff_hz
    + half the transition band = min(Fi, Fo) / 2) is at least 60 dB down, aliased or not"""
    fo, fi = 48000, num / den
    cut = rm.clean_cutoff(fi, fo, T, beta)
    edge = cut + 0.5 * rm.transition_hz(fi, T, beta)
    assert abs(edge - 0.5 * min(fi, fo)) < 1e-6
    n = np.arange(int(0.05 * fi))
    gains = []
    for f in (1000.0, edge + 500.0):
        x = np.sin(2 * np.pi * f * n / fi).astype(np.float32)
        y = rm.resample(x, num, den, fo, T, beta, cut)
        y = y[4 * T:len(y) - 4 * T]                       # past the filter's transient
        gains.append(10 * np.log10(np.mean(y ** 2) / 0.5))
    print("rsmp tones %g -> %d Hz, T = %d: cutoff %.1f Hz, 1 kHz %+.3f dB, %.0f Hz %.1f dB" % (fi, fo, T, cut, gains[0],
                                                                                               edge + 500.0, gains[1]))
    assert abs(gains[0]) < 0.1 and gains[1] < -60.0


def _frames(count, seed, size=30):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, size, dtype=np.uint8)) for _ in range(count)]


def _decode(x):
    a = ko.Afsk()
    a.push(np.asarray(x, np.float32))
    got = a.frames()
    a.close()
    return got


@pytest.mark.parametrize("num,den,T,beta", [(50000, 1, 32, 3.0), (10000000, 256, 32, 3.0), (31250, 1, 16, 2.0)])
def test_afsk_decodes_after_resampling_and_not_before(num, den, T, beta):
    frames = _frames(6, 7)
    sent = [f + ax25_fcs(f) for f in frames]
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    x = afsk_audio(afsk_bits(frames) + flag * 12, samprate=num / den)
    assert _decode(x) == [], "packet.c's decoder reads 48 kHz audio only"
    y = rm.resample(x, num, den, 48000, T, beta)
    assert _decode(y) == sent


# ---- behind a receiver bank: two FM channels at 50 kHz carrying AFSK, shared with tests/test_gpu_rsmp.py
GEOM = dict(samprate=200000, L=512, M=513, D=4)
CARRIERS = (30000.0, -45000.0)
DEVIATION = 3000.0
PER_CALL = 49
RSMP_T, RSMP_BETA = 32, 3.0


def fm_plan():
    """flat FM channels: the test signal has no pre-emphasis, and through fm.c's de-emphasis its 2200 Hz tone comes out so far
    below the 1200 Hz one that packet.c's decoder sits on the edge (it then loses all four frames or none to a change of 1e-5
    in the audio); from flat channels it decodes all of them under thirty perturbations of 1e-7 .. 1e-2 of the peak"""
    return [dict(demod="fm", low=-8000.0, high=8000.0, second_lo=-f, flat=1) for f in CARRIERS]


@functools.lru_cache(maxsize=None)
def fm_afsk_case():
    """-> (iq complex64 [nblocks L], frames sent per channel with their FCS, nblocks): two FM carriers, each modulated by
    the AFSK audio of four 30-byte frames behind a lead-in of flags, with a little receiver noise"""
    fs, L = GEOM["samprate"], GEOM["L"]
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    frames = [_frames(4, 20 + c) for c in range(len(CARRIERS))]
    audio = [afsk_audio(flag * (24 + 3 * c) + afsk_bits(f) + flag * 16, samprate=float(fs), amp=1.0) for c, f in enumerate(frames)]
    nblocks = -(-max(len(a) for a in audio) // (L * PER_CALL)) * PER_CALL
    n = nblocks * L
    t = np.arange(n)
    iq = np.zeros(n, np.complex128)
    for f, a in zip(CARRIERS, audio):
        a = np.concatenate([a.astype(np.float64), np.zeros(n - len(a))])
        iq += 0.2 * np.exp(1j * (2 * np.pi * f * t / fs + 2 * np.pi * DEVIATION * np.cumsum(a) / fs))
    rng = np.random.default_rng(3)
    iq += 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq, [[f + ax25_fcs(f) for f in fr] for fr in frames], nblocks


def test_afsk_through_the_oracles_receiver_and_the_model():
    """run_oracle (the reference's FM chain at 50 kHz) -> the model at 24 / 25 -> the oracle's Afsk: every frame sent, also with
    the audio disturbed by 1e-5 and 1e-3 of its peak (the GPU's receiver and decoder differ from the oracle's in the last bits)"""
    iq, sent, nblocks = fm_afsk_case()
    want = run_oracle(fm_plan(), GEOM, iq, nblocks)
    rng = np.random.default_rng(4)
    for c, (auds, _, _) in enumerate(want):
        x = np.concatenate(auds)
        assert len(x) == nblocks * GEOM["L"] // GEOM["D"]
        assert _decode(x) == []
        y = rm.resample(x, GEOM["samprate"], GEOM["D"], 48000, RSMP_T, RSMP_BETA)
        assert _decode(y) == sent[c], c
        for eps in (1e-5, 1e-3):
            assert _decode(y + eps * np.abs(y).max() * rng.standard_normal(len(y))) == sent[c], (c, eps)
