"""The spectrum bank's CPU model (tests/spec_model.py) against the readings the ABI promises (include/ka9q_hip.h,
kq_spec_*): a tone on a bin centre reads A^2, white noise reads N0 enbw_bins bin_bw, the decimator keeps aliases 80 dB
down, rows do not depend on how the stream is split, and plan() picks (decimate, fft_size)."""
import numpy as np
import pytest

import spec_model as sm
from ka9q_sdr_amd.spectrum import plan

FS = 1000000


def _tone(A, f, n, fs=FS):
    return A * np.exp(2j * np.pi * f / fs * np.arange(n))


@pytest.mark.parametrize("Nf,k,center", [(1024, 37, 12345.0), (960, -200, -250000.0), (16384, 5000, 0.0)])
def test_tone_on_bin_centre_reads_A2_at_Dz1(Nf, k, center):
    p = sm.params(center=center, fft_size=Nf, average=2)
    A = 0.3
    rows, _ = sm.analyzer_rows(_tone(A, center + k * FS / Nf, 6 * Nf), p, FS)
    assert len(rows) >= 2
    assert np.max(np.abs(rows[:, Nf // 2 + k] / A ** 2 - 1)) < 1e-9


@pytest.mark.parametrize("Dz,Nf", [(8, 512), (25, 400), (64, 256)])
def test_tone_on_bin_centre_reads_A2_over_kept_bins_when_zoomed(Dz, Nf):
    p = sm.params(center=-20000.0, decimate=Dz, fft_size=Nf, average=1)
    B, bw, A = p["bins"], FS / (Dz * Nf), 0.5
    s0 = 24 * Dz                 # the analyzer starts once the tone has filled the decimator's taps
    n = s0 + (Nf + 1) * Dz
    for k in (-B // 2, -B // 3, -1, 0, 7, B // 4, B // 2 - 1):
        rows, _ = sm.analyzer_rows(_tone(A, p["center"] + k * bw, n), p, FS, s0=s0)
        err_db = 10 * np.log10(rows[:, B // 2 + k] / A ** 2)
        assert np.max(np.abs(err_db)) < 0.01, (k, err_db)


@pytest.mark.parametrize("Dz,Nf,K", [(1, 1024, 8), (16, 512, 8)])
def test_white_noise_reads_N0_enbw_bin_bw(Dz, Nf, K):
    """complex white noise of power s2 per sample has N0 = s2 / Fs; the mean reading over every kept bin of every row is
    N0 enbw_bins bin_bw.  Bound: the readings average R K frames (50 % overlap) of B bins, about R K B / (2 enbw_bins)
    independent exponential variates, whose mean has relative spread 1 / sqrt of that; 5 of those."""
    rng = np.random.default_rng(7)
    p = sm.params(center=3000.0, decimate=Dz, fft_size=Nf, average=K)
    s2 = 0.02
    n = (24 * Dz) + Dz * Nf * (K + 1) * 6
    x = np.sqrt(s2 / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    rows, _ = sm.analyzer_rows(x, p, FS)
    inf = sm.info(p, FS)
    want = s2 / FS * inf["enbw_bins"] * inf["bin_bw"]
    eff = rows.size * K / (2 * inf["enbw_bins"])
    assert abs(rows.mean() / want - 1) < 5 / np.sqrt(eff), (rows.mean() / want, eff)


@pytest.mark.parametrize("Dz,Nf", [(8, 512), (25, 400), (256, 64)])
def test_alias_from_beyond_five_eighths_is_80_dB_down(Dz, Nf):
    """a tone one bin beyond 5/8 of the decimated rate folds onto bin -3 Nf / 8 + 1, inside the kept bins"""
    p = sm.params(center=1000.0, decimate=Dz, fft_size=Nf, average=1)
    B, bw = p["bins"], FS / (Dz * Nf)
    k_in = -3 * Nf // 8 + 1
    s0 = 24 * Dz
    n = s0 + (Nf + 1) * Dz
    ref, _ = sm.analyzer_rows(_tone(1.0, p["center"] + k_in * bw, n), p, FS, s0=s0)
    ali, _ = sm.analyzer_rows(_tone(1.0, p["center"] + (k_in + Nf) * bw, n), p, FS, s0=s0)
    assert abs(10 * np.log10(ref[0, B // 2 + k_in])) < 0.01
    assert 10 * np.log10(ali[0].max() / ref[0, B // 2 + k_in]) <= -80


def test_rows_do_not_depend_on_the_split():
    """the model evaluates the whole stream in double (transform lengths follow the stream length), so its rows agree to
    1e-12; the bank's agree bit for bit (tests/test_gpu_spectrum.py)"""
    rng = np.random.default_rng(3)
    x = (rng.integers(-3000, 3000, (40000, 2))).astype(np.int16)
    ps = [sm.params(center=1e5, sweep=2e5, decimate=8, fft_size=256, average=3),
          sm.params(center=-4e5, fft_size=1000, hop=333, average=2)]
    whole, split = sm.SpecModel(FS, max_rows=1000, gain_factor=0.5), sm.SpecModel(FS, max_rows=1000, gain_factor=0.5)
    for i, p in enumerate(ps):
        whole.set(i, p)
        split.set(i, p)
    whole.process(x)
    cuts = [0, 1, 3, 10, 500, 501, 20000, 40000]
    for a, b in zip(cuts[:-1], cuts[1:]):
        split.process(x[a:b])
    for i in range(len(ps)):
        rw, sw, gw = whole.pull(i)
        rs, ss, gs = split.pull(i)
        assert len(rw) > 3 and np.array_equal(sw, ss) and np.array_equal(gw, gs)
        assert np.max(np.abs(rw - rs) / rw.max(axis=1, keepdims=True)) < 1e-12


def test_sweep_follows_a_chirp():
    """an analyzer swept at the chirp's rate sees it stand still on one bin"""
    rate, f0, A = 4e6, 50000.0, 0.7      # Hz/s
    n = np.arange(200000)
    x = A * np.exp(2j * np.pi * (f0 / FS * n + 0.5 * rate / FS ** 2 * n * n))
    p = sm.params(center=f0, sweep=rate, decimate=16, fft_size=256, average=1)
    rows, _ = sm.analyzer_rows(x, p, FS)
    B = p["bins"]
    assert np.all(np.argmax(rows, axis=1) == B // 2)
    assert np.max(np.abs(10 * np.log10(rows[:, B // 2] / A ** 2))) < 0.01


def test_plan():
    assert plan(10000000, 100, 3000) == (25, 4000)
    assert plan(10000000, 10000000 / 16384, 16384) == (1, 16384)
    dz, nf = plan(1000000, 10, 4096)                 # 100000 = Dz Nf
    assert dz * nf == 100000 and dz <= 256 and 4 * 4096 <= 3 * nf
    assert plan(48000, 46.875, 1024) == (1, 1024)
    with pytest.raises(ValueError, match="not an integer"):
        plan(10000000, 3, 1000)                       # 10e6 / 3 is no integer
    with pytest.raises(ValueError, match="no decimate"):
        plan(10000000, 1, 1000)                       # 10^7 = Dz Nf needs Dz > 256 or Nf > 16384
    with pytest.raises(ValueError, match="no decimate"):
        plan(1000000, 500, 2002)                      # 2000 = Dz Nf: no Nf of 2000 keeps 2002 bins
    assert plan(1000000, 500, 1500) == (1, 2000)
