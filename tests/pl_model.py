"""The PL slave and the PL tone tracker of the FM demodulator (pltask, fm.c:201-277) restated in float64, and the cases the
sample-level PL tests share.

The slave is a REAL -> REAL overlap-save filter on the audio master's spectrum that decimates by N_dec / PL_N (32 where 32
divides the sizes): windows of N_dec detected samples, the first M_dec - 1 of them the end of the window before; bins
0 ... PL_N/2 of the window's transform times the PL response; a Hermitian inverse transform of PL_N points whose last PL_L
outputs are the block's PL samples (filter.c:140,206-208,250).  The tracker appends them to a ring of 16384 samples and, after
every 512 new ones, transforms the ring as it lies in memory and reads the tone off the peak bin (fm.c:236-277).

`status.plfreq` is the only thing the tracker shows, and a spectral line survives almost anything done to a block's samples;
the slave is therefore compared sample by sample (kq_bank_pull_pl_samples against the oracle's pl_filter->output_r), and the
MUTANTS below are the wrong slaves that comparison has to see."""
import functools

import numpy as np

import kq_oracle as ko
from common import oracle_cfg, rel_rms

PL_DECIMATE = 32
RING = (1 << 19) // PL_DECIMATE          # fm.c:225


def pl_sizes(n_dec, m_dec):
    """-> PL_N, PL_L (fm.c:203-204; create_filter_output truncates where 32 does not divide, filter.c:103-107,116)"""
    return n_dec // PL_DECIMATE, (n_dec - m_dec + 1) // PL_DECIMATE


def pl_response(n_dec, m_dec, dsamprate):
    """The PL low-pass as the demodulators design it: bins with 0 < f < 300 Hz, windowed by the oracle's window_rfilter with
    Kaiser beta 2.0 (fm.c:207-218)."""
    pl_n, pl_l = pl_sizes(n_dec, m_dec)
    r = np.zeros(pl_n // 2 + 1, np.complex64)
    for j in range(pl_n // 2 + 1):
        f = np.float32(j) * np.float32(dsamprate) / np.float32(n_dec)
        if 0 < f < 300:
            r[j] = 1
    ko.lib().kqo_window_rfilter(pl_l, pl_n - pl_l + 1, r.ctypes.data, 2.0)
    return r.astype(np.complex128)


MUTANTS = ("no_transform", "time_reversed", "first_kept", "no_response")


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def pl_slave(stream, n_dec, m_dec, resp, mutant=None):
    """stream: the detected samples of a channel, block after block (a flat channel's audio) -> PL samples [nblocks][PL_L].
    mutant: None, or one of MUTANTS --
      no_transform    the inverse transform runs no butterflies: the output buffer still holds the Hermitian-extended
                      spectrum in the order the transform wants its input (bit-reversed for a power of two; natural otherwise)
      time_reversed   the inverse transform with the forward sign: y[-n mod PL_N]
      first_kept      the first PL_L outputs kept instead of the last
      no_response     the spectrum not multiplied by the PL response"""
    assert mutant is None or mutant in MUTANTS
    pl_n, pl_l = pl_sizes(n_dec, m_dec)
    al = n_dec - m_dec + 1
    nblocks = len(stream) // al
    x = np.concatenate([np.zeros(m_dec - 1), np.asarray(stream, np.float64)])
    out = np.zeros((nblocks, pl_l))
    for b in range(nblocks):
        spec = np.fft.rfft(x[b * al:b * al + n_dec])
        g = spec[:pl_n // 2 + 1].copy()
        if mutant != "no_response":
            g *= resp
        g[0] = g[0].real             # the c2r transform ignores the imaginary parts of DC and Nyquist (filter.c:250)
        g[-1] = g[-1].real
        if mutant == "no_transform":
            ext = np.concatenate([g, np.conj(g[-2:0:-1])])
            bits = pl_n.bit_length() - 1
            if pl_n == 1 << bits:
                y = np.array([ext[_bitrev(p, bits)].real for p in range(pl_n)])
            else:
                y = ext.real
        else:
            y = np.fft.irfft(g, pl_n) * pl_n        # unnormalised, as fftwf_plan_dft_c2r_1d
        if mutant == "time_reversed":
            y = y[(-np.arange(pl_n)) % pl_n]
        out[b] = y[:pl_l] if mutant == "first_kept" else y[pl_n - pl_l:]
    return out


def pl_track(blocks, dsamprate):
    """PL samples block by block -> plfreq after every block (fm.c:236-277; NaN until the first reading)"""
    ring = np.zeros(RING)
    ptr = last = 0
    plfreq = np.float32(np.nan)
    pl_samprate = np.float32(dsamprate) / np.float32(PL_DECIMATE)
    out = []
    for y in blocks:
        idx = (ptr + np.arange(len(y))) % RING
        ring[idx] = y
        ptr = (ptr + len(y)) % RING
        last += len(y)
        if last >= 512:
            last = 0
            e = np.abs(np.fft.rfft(ring)[1:RING // 2]) ** 2          # skip DC (fm.c:260)
            peak = int(np.argmax(e))
            if e[peak] > 0 and e[peak] > 0.01 * e.sum():
                f = np.float32(peak + 1) * pl_samprate / np.float32(RING)
                if 67 < f < 255:
                    plfreq = f
            else:
                plfreq = np.float32(np.nan)
        out.append(float(plfreq))
    return out


# ---- the cases: the smallest shapes that reach each path of the slave (N never beyond 8232) ------------------------------
# (name, samprate, L, M, D, blocks per call, tone).  From (N_dec, D, k): M = k D + 1, L = (N_dec - k) D, samprate = 48000 D.
def _ndk(nd, D, k, tone, per_call=11):
    return ("ndec%d_D%d_k%d" % (nd, D, k), 48000 * D, (nd - k) * D, k * D + 1, D, per_call, tone)


CASES = [
    # a power-of-two PL slave under a master with a factor 3, 5 or 7
    _ndk(270, 8, 110, 88.5), _ndk(280, 8, 120, 131.8), _ndk(540, 4, 220, 88.5), _ndk(1050, 4, 410, 131.8),   # (1050: 256 threads)
    _ndk(2058, 2, 778, 88.5), _ndk(4116, 2, 1556, 131.8),
    # a PL slave with such a factor itself: 12 and 60 points
    _ndk(400, 4, 160, 88.5), _ndk(1920, 8, 960, 131.8),
    # a power-of-two master: cfg 2's geometry in calls of 37 blocks, so that the pairs of blocks of the register kernel straddle
    # the calls; a 512-point master on the LDS transform; cfg 1's geometry
    ("cfg2", 2000000, 8192, 8193, 64, 37, 88.5), _ndk(512, 4, 256, 131.8), ("cfg1", 192000, 8192, 8193, 4, 11, 88.5),
]
CASE_IDS = [c[0] for c in CASES]
SECONDS = 1.25                     # three ring transforms


def case_signal(case):
    """-> geom, iq, nblocks, plan: the usual voice (1 kHz, 3 rad) and a PL tone (6 rad) on a carrier at 0.1 fs, 30 dB in-channel
    SNR; a de-emphasised and a flat FM channel"""
    name, fs, L, M, D, per_call, tone = case
    geom = dict(samprate=fs, L=L, M=M, D=D)
    nblocks = int(np.ceil(SECONDS * fs / L))
    t = np.arange(nblocks * L) / fs
    fc = 0.1 * fs
    rng = np.random.default_rng(L + M)
    ph = 2 * np.pi * fc * t + 3.0 * np.sin(2 * np.pi * 1000.0 * t) + 6.0 * np.sin(2 * np.pi * tone * t)
    sigma = 0.1 * 10 ** (-30 / 20) / np.sqrt(2 * 16000.0 / fs)
    iq = (0.1 * np.exp(1j * ph) + sigma / np.sqrt(2) * (rng.standard_normal(len(t)) + 1j * rng.standard_normal(len(t)))).astype(np.complex64)
    plan = [dict(demod="fm", low=-8000.0, high=8000.0, second_lo=-fc),
            dict(demod="fm", low=-8000.0, high=8000.0, second_lo=-fc, flat=1)]
    return geom, iq, nblocks, plan


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """The oracle and the model on a case, computed once and shared (read only): dict with geom, iq, nblocks, plan, want (per
    channel: audio, status, filter output and PL samples of every block), n_dec, m_dec, dsamprate, resp, model (the model's PL
    samples, fed from the oracle's flat-channel audio) and e_ref = the relative RMS error of the oracle's PL samples against them."""
    geom, iq, nblocks, plan = case_signal(case)
    L, M, D, fs = geom["L"], geom["M"], geom["D"], geom["samprate"]
    want = [ko.run_chain(oracle_cfg(p, fs, L, M, D, 0), iq.reshape(nblocks, L), want_filt=True, want_pl=True) for p in plan]
    n_dec, m_dec, dsamprate = (L + M - 1) // D, (M - 1) // D + 1, fs / D
    resp = pl_response(n_dec, m_dec, dsamprate)
    stream = np.concatenate(want[1][0])
    model = pl_slave(stream, n_dec, m_dec, resp)
    e_ref = rel_rms(np.concatenate(want[1][3]), model.ravel())
    return dict(geom=geom, iq=iq, nblocks=nblocks, plan=plan, want=want, n_dec=n_dec, m_dec=m_dec, dsamprate=dsamprate,
                resp=resp, stream=stream, model=model, e_ref=e_ref)
