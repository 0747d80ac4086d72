"""The CPU model of the modulator bank (tests/mod_model.py) against independent float64 math: linear convolution of the
zero-stuffed audio with the response's M-tap impulse response, times a closed-form swept phasor."""
import numpy as np
import pytest

import mod_model as mm
from common import rel_rms

GEOMS = [dict(samprate=192000, L=4096, M=4097, interp=4),     # modulate.c:25,109-112
         dict(samprate=240000, L=4800, M=4801, interp=5)]     # N = 9600 = 2^7 3 5^2


def _direct(g, st, audio, nblocks):
    Fs, L, M, I = g["samprate"], g["L"], g["M"], g["interp"]
    N = L + M - 1
    h = np.fft.ifft(mm.design_response(Fs, L, M, I, st["low"], st["high"], st["kaiser_beta"]).astype(np.complex128)) * N
    assert np.abs(h[M:]).max() < 1e-6 * np.abs(h).max()           # the impulse response lies in the first M taps
    x = np.zeros(nblocks * L)
    x[::I] = audio[:nblocks * L // I]
    y = np.convolve(x, h[:M])[:nblocks * L]                        # zero history before the first block (filter.c:76)
    n = np.arange(nblocks * L, dtype=np.float64)
    f, r = st["frequency"] / Fs, st["sweep"] / (float(Fs) * Fs)
    ph = np.exp(2j * np.pi * (n * f + r * n * (n - 1) / 2))
    if st["mod_type"] == 1:
        bb = np.exp(2j * np.pi * (st["deviation"] / Fs) * np.cumsum(y.real))
    else:
        bb = y + st["carrier"]
    return bb * ph * 10 ** (st["amplitude_dbfs"] / 20)


def _audio(g, nblocks, seed):
    rng = np.random.default_rng(seed)
    n = nblocks * g["L"] // g["interp"]
    t = np.arange(n) / (g["samprate"] / g["interp"])
    return (0.4 * np.sin(2 * np.pi * 1100 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("g", GEOMS, ids=["192k", "240k"])
@pytest.mark.parametrize("st", [mm.station("am"), mm.station("usb", frequency=-20000.5, sweep=3000.0),
                                mm.station("lsb", frequency=33333.3), mm.station("ame", amplitude_dbfs=-3.0),
                                mm.station("fm", frequency=40000.0, deviation=2500.0)],
                         ids=["am", "usb-swept", "lsb", "ame", "fm"])
def test_oracle_station_matches_direct_math(g, st):
    nblocks = 3
    a = _audio(g, nblocks, 1)
    ref = mm.OracleStation(g["samprate"], g["L"], g["M"], g["interp"], st)
    La = g["L"] // g["interp"]
    got = np.concatenate([ref.block(a[b * La:(b + 1) * La]) for b in range(nblocks)])
    ref.close()
    assert rel_rms(got, _direct(g, st, a, nblocks)) < 1e-5


@pytest.mark.parametrize("g", GEOMS, ids=["192k", "240k"])
def test_bank_model_matches_oracle_station(g):
    """the batched float64 model = one OracleStation per station, including a retune (phase-continuous) and a mode change"""
    nblocks = 2
    La = g["L"] // g["interp"]
    plan = [mm.station("am", frequency=31000.0), mm.station("usb", frequency=-45000.0, sweep=-900.0),
            mm.station("fm", frequency=7000.0)]
    pcm = np.stack([_audio(g, 2 * nblocks, s) for s in range(3)])
    model = mm.BankModel(**g)
    refs = [mm.OracleStation(g["samprate"], g["L"], g["M"], g["interp"], st) for st in plan]
    for s, st in enumerate(plan):
        model.set_station(s, st)
    for half in range(2):
        if half == 1:
            new = [dict(plan[0], frequency=32000.0, amplitude_dbfs=-30.0), mm.station("lsb", frequency=-45000.0), plan[2]]
            for s, st in enumerate(new):
                model.set_station(s, st)
                refs[s].set(st)
        chunk = pcm[:, half * nblocks * La:(half + 1) * nblocks * La]
        want, each = model.process(chunk, nblocks, per_station=True)
        for s in range(3):
            got = np.concatenate([refs[s].block(chunk[s, b * La:(b + 1) * La]) for b in range(nblocks)])
            assert rel_rms(got, each[s]) < 1e-5, (half, s)
    for r in refs:
        r.close()


def test_to_s16_truncates_and_saturates():
    x = np.array([0.5, -0.5, 1.5, -1.5, 1e-6, -0.99999], np.float32).astype(np.complex64)
    got = mm.to_s16(x)[:, 0]
    assert list(got) == [16383, -16383, 32767, -32768, 0, -32766]
