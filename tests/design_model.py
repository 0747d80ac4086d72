"""The reference's filter response design (filter.c:282-546, fm.c:54-66) restated in float64, the case tables the design
tests share, and the bars they hold the oracle and the device to.

Plain numpy, no project code.  Every function states the reference's PROCEDURE, not an idealisation of it: the in-place
rotation of the taps (n descending: with M >= 2 L the first taps are formed from slots the loop has already windowed and
scaled), c2r semantics of the REAL design (the imaginary parts of DC and Nyquist are ignored), bin frequencies and band
comparisons in float32.  Only the arithmetic is float64, so that the float32 implementations -- the oracle on the CPU, the
design kernels on the device -- can each be measured against it.

The keyword arguments that default to the reference's behaviour are MUTANTS: the wrong designs a comparison of responses has
to see.  tests/test_design_model.py shows that each sensitive case below is at least 10 x its family's device bar away from
its mutant; tests/test_gpu_design.py runs the same cases on the device.
"""
import functools

import numpy as np

# ---- bars -------------------------------------------------------------------------------------------------------------------
# BASELINE: the oracle's own worst error against this model over the family's case table below -- oracle vs float64, CPU,
# measured 2026-10-19 by tests/test_design_model.py (which asserts that the oracle still stays within it) and rounded up to
# two digits.  Response families: max |oracle - model| over all bins / max |model|; kaiser: max absolute difference of the
# taps (the window peaks at 1); noise_gain: relative.
# BAR: what the device is held to, DEVICE_FACTOR x the baseline.  The device runs the same float procedure as the oracle with a
# differently ordered transform (register / LDS radix stages against the oracle's radix-2 recursion); the factor covers the
# ordering.  Every defect of interest stays 10 x above the bar: one bin is >= 1e-2 of the peak, the in-place rule >= 6e-5 at
# the sensitive cases.
DEVICE_FACTOR = 4.0
BASELINE = {
    "kaiser": 2.6e-6,               # make_kaiser, all of KAISER_M x KAISER_BETA (the worst at beta = 10)
    "window_filter": 5.4e-7,        # window_filter, beta <= 3
    "window_filter_b9": 1.2e-6,     # window_filter, beta = 9
    "window_rfilter": 5.3e-7,       # window_rfilter, beta <= 3
    "window_rfilter_b9": 9.9e-7,    # window_rfilter, beta = 9
    "band": 3.0e-7,                 # set_filter's response, beta = 3 (band_edges)
    "band_bank": 6.4e-7,              # set_filter's response at the edges and betas (0, 1, 3, 5) of the bank plans
    "noise_gain": 2.4e-5,           # set_filter's noise gain (a float sum over N_dec bins in sequence: the worst at N_dec = 1920)
    "audio": 2.1e-7,                # the FM audio response
}
BAR = {k: DEVICE_FACTOR * v for k, v in BASELINE.items()}
SENSITIVITY_FACTOR = 10.0   # a sensitive case differs from its mutant by at least this many bars


def bessel_i0(x):
    """filter.c:282-293: sum_k (x^2/4)^k / (k!)^2, cut off where a term drops below 1e-12 of the sum or after 40 terms"""
    x = np.asarray(x, np.float64)
    q = 0.25 * x * x
    term = q.copy()
    total = 1.0 + q
    live = np.ones(q.shape, bool)
    for k in range(2, 40):
        term = term * (q / (k * k))
        total = np.where(live, total + term, total)
        live = live & ~(term < 1e-12 * total)
    return total


def kaiser(M, beta, denom=None):
    """filter.c:337-357: I0(pi beta sqrt(1 - p^2)) / I0(pi beta), p = 2 m / (M - 1) - 1, m = min(n, M - 1 - n); M = 1: [1.0].
    Mutant denom = M: a window of length M + 1 sampled at its first M points."""
    n = np.arange(M, dtype=np.float64)
    if denom is None:
        if M == 1:
            return np.ones(1)
        p = 2.0 * np.minimum(n, M - 1 - n) / (M - 1) - 1.0
    else:
        p = 2.0 * n / denom - 1.0
    arg = np.pi * float(beta)
    return bessel_i0(arg * np.sqrt(1.0 - p * p)) / bessel_i0(arg)


def _rotate_window_scale(buf, L, M, w, in_place):
    """filter.c:389-390 / 445-446: for n = M-1 .. 0: buf[n] = buf[(n - M/2 + N) % N] * w[n] / N, IN PLACE, then zero from M on.
    Mutant in_place = False: every tap from the untouched time-domain buffer."""
    N = L + M - 1
    h = M // 2
    work = buf.copy()
    # n >= M/2: the source n - M/2 lies below n, where the descending loop has not been yet
    work[h:M] = buf[0:M - h] * w[h:M] / N
    for n in range(h - 1, -1, -1):          # the source N - M/2 + n lies above n: already rewritten if it is below M
        src = (n - h + N) % N
        work[n] = (work[src] if in_place else buf[src]) * w[n] / N
    work[M:] = 0
    return work


def window_filter(L, M, resp, beta, in_place=True, window=None):
    """filter.c:365-415 on N = L + M - 1 complex bins.  `window`: taps to use instead of kaiser(M, beta) (a mutant window)."""
    N = L + M - 1
    resp = np.asarray(resp, np.complex128)
    assert resp.shape == (N,)
    buf = np.fft.ifft(resp) * N                       # the unnormalised backward transform
    w = kaiser(M, beta) if window is None else np.asarray(window, np.float64)
    return np.fft.fft(_rotate_window_scale(buf, L, M, w, in_place))


def window_rfilter(L, M, resp, beta, in_place=True, keep_dc_imag=False):
    """filter.c:420-469 on N/2 + 1 bins: a real time buffer by a c2r transform (the imaginary parts of DC and Nyquist are
    ignored), the same loop, an r2c transform; returns N/2 + 1 bins.
    Mutant keep_dc_imag: DC and Nyquist go through a complex transform as they are and the taps carry what that leaves."""
    N = L + M - 1
    resp = np.asarray(resp, np.complex128)
    assert resp.shape == (N // 2 + 1,)
    full = np.zeros(N, np.complex128)                 # the Hermitian extension a c2r transform stands for
    full[:N // 2 + 1] = resp
    k = np.arange(1, (N + 1) // 2)
    full[N - k] = np.conj(resp[k])
    if not keep_dc_imag:
        full[0] = full[0].real
        if N % 2 == 0:
            full[N // 2] = full[N // 2].real
    buf = np.fft.ifft(full) * N
    if not keep_dc_imag:
        buf = buf.real.astype(np.complex128)
    taps = _rotate_window_scale(buf, L, M, kaiser(M, beta), in_place)
    return np.fft.fft(taps)[:N // 2 + 1]


def rewritten_taps(L, M):
    """How many taps the in-place loop forms from slots it has already written (none while L > M/2)"""
    N, h = L + M - 1, M // 2
    return sum(1 for n in range(h) if N - h + n < M)


def signed_bins(n_dec):
    n = np.arange(n_dec)
    return np.where(n <= n_dec // 2, n, n - n_dec)


def band_target(N, L_dec, M_dec, low, high, two_sided, extra_bin=0):
    """set_filter's target (filter.c:518-535): bin n of N_dec lies at float32(signed n) / float32(N_dec) and is in the band
    where low <= f <= high, compared in float32; gain float32(1 / float32(N)), times 1/sqrt(2) where two sidebands add (the
    product with the double M_SQRT1_2, rounded to float).
    Mutant extra_bin = +1 / -1: one bin more above the high / below the low edge."""
    n_dec = L_dec + M_dec - 1
    k = signed_bins(n_dec)
    f = k.astype(np.float32) / np.float32(n_dec)
    inside = (f >= np.float32(low)) & (f <= np.float32(high))
    if extra_bin > 0:
        above = k[f > np.float32(high)]
        if above.size:
            inside = inside | (k == above.min())
    elif extra_bin < 0:
        below = k[f < np.float32(low)]
        if below.size:
            inside = inside | (k == below.max())
    gain = np.float32(1.0) / np.float32(N)
    if two_sided:
        gain = np.float32(np.float64(gain) * np.sqrt(0.5))
    return np.where(inside, np.float64(gain), 0.0).astype(np.complex128)


def noise_gain(N, resp, two_sided, real_real=False):
    """filter.c:472-497: (2 if two sidebands add) N sum |H|^2, over N_dec / 2 + 1 bins only for a REAL-in / REAL-out slave"""
    resp = np.asarray(resp)
    if real_real:
        resp = resp[:len(resp) // 2 + 1]
    return (2.0 if two_sided else 1.0) * N * float(np.sum(np.abs(resp) ** 2))


def set_filter(N, L_dec, M_dec, low, high, beta, two_sided, extra_bin=0, in_place=True):
    """filter.c:500-546 -> (response of N_dec bins, noise gain)"""
    r = window_filter(L_dec, M_dec, band_target(N, L_dec, M_dec, low, high, two_sided, extra_bin), beta, in_place=in_place)
    return r, noise_gain(N, r, two_sided)


def deemph_target(AL, AM, dsamprate):
    """fm.c:39-63: bins 0 .. AN/2 at f = float32(j) * dsamprate / AN (in float); 10 / AN * 300 / f where 300 <= f <= 6000"""
    AN = AL + AM - 1
    gain = np.float32(10.0 / AN)
    j = np.arange(AN // 2 + 1)
    f = j.astype(np.float32) * np.float32(dsamprate) / np.float32(AN)
    inside = (f >= np.float32(300)) & (f <= np.float32(6000))
    r = np.zeros(AN // 2 + 1, np.complex128)
    r[inside] = np.float64(gain) * 300.0 / f[inside].astype(np.float64)
    return r


def audio_response(AL, AM, dsamprate, beta, in_place=True):
    """fm.c:54-66: the FM audio filter, window_rfilter of the de-emphasis target"""
    return window_rfilter(AL, AM, deemph_target(AL, AM, dsamprate), beta, in_place=in_place)


def rel_peak(got, want):
    """max |got - want| over all bins / max |want|"""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# ---- case tables ------------------------------------------------------------------------------------------------------------
KAISER_M = (1, 2, 3, 64, 129, 257, 4353)              # 257: past one 256-thread block of the window kernel
KAISER_BETA = (0.0, 0.5, 3.0, 7.5, 10.0)
# the Kaiser cases the denominator mutant shows to be sensitive (beta = 0 is all ones whatever the denominator)
KAISER_SENSITIVE = tuple((M, b) for M in KAISER_M for b in KAISER_BETA if b > 0)

# (L, M) of window_filter / window_rfilter, N = L + M - 1
WINDOW_SHAPES = (
    (1, 2),          # N = 2
    (32, 33),
    (128, 129),
    (512, 513),      # N = 1024: the first 256-thread launch
    (511, 514),      # even M
    (960, 65),
    (65, 128),       # N = 192 either side of M = 2 L: no rewritten tap ...
    (64, 129),       # ... and one
    (320, 705),
    (640, 1409),     # an FM audio filter (fm.c:64): blocks of 640 samples, 1409 taps
    (1024, 3073),    # M = 3 L + 1
    (256, 1793),     # M = 7 L + 1
    (960, 961),      # N = 1920 = 2^7 3 5
    (896, 897),      # N = 1792 = 2^8 7
    (4800, 4801),    # N = 9600 = 2^7 3 5^2
    (8192, 8193),    # N = 16384: the most one workgroup's LDS holds
)
WINDOW_BETA = (0.0, 3.0)
WINDOW_B9_SHAPES = ((128, 129), (960, 961), (8192, 8193))      # beta = 9: shapes without rewritten taps
# the shapes with rewritten taps (rewritten_taps > 0), and the (L, M, beta) at which the in-place rule is 10 bars strong: all
# of them at beta 0 and 3, but for the single rewritten tap of (64, 129) under the beta = 3 window in the REAL design (its
# real part alone: 5e-6 of the peak)
INPLACE_SHAPES = ((1, 2), (64, 129), (320, 705), (640, 1409), (1024, 3073), (256, 1793))
INPLACE_SENSITIVE = tuple((L, M, b) for (L, M) in INPLACE_SHAPES for b in WINDOW_BETA)
INPLACE_SENSITIVE_REAL = tuple(c for c in INPLACE_SENSITIVE if c != (64, 129, 3.0))

# set_filter through the one-channel surface: master (L, M), decimate D
BAND_GEOMETRIES = (
    (32, 33, 1),
    (96, 97, 1),         # N_dec = 192
    (512, 513, 4),
    (4800, 4801, 5),     # N_dec = 1920
    (1024, 3073, 8),     # N_dec = 512, M_dec = 385 >= 2 L_dec: rewritten taps
)
BAND_BETA = 3.0
OUT_COMPLEX, OUT_CROSS_CONJ, OUT_REAL = 1, 2, 3       # enum filtertype (filter.h)
BAND_OUT_TYPES = (OUT_COMPLEX, OUT_CROSS_CONJ, OUT_REAL)


def band_geometry(L, M, D):
    """-> N, L_dec, M_dec, N_dec (filter.c:116, 514)"""
    N = L + M - 1
    return N, L // D, (M - 1) // D + 1, N // D


def band_edges(n_dec):
    """-> list of (low, high, what): edges exactly on bins -- 16 evenly spaced signed bins and the ends of both halves, one-bin
    and four-bin bands -- each as it is, with `low` one float above its bin and with `high` one float below (the edge bin then
    drops out); low > high; the whole circle."""
    ks = sorted(set(int(round(v)) for v in np.linspace(-n_dec // 2 + 1, n_dec // 2, 16)) | {-n_dec // 2 + 1, -1, 0, 1, n_dec // 2})
    out = []
    for k in ks:
        for width in (0, 3):
            low = np.float32(k) / np.float32(n_dec)
            high = np.float32(k + width) / np.float32(n_dec)
            out.append((float(low), float(high), "k %d w %d" % (k, width)))
            out.append((float(np.nextafter(low, np.float32(np.inf))), float(high), "k %d w %d low+" % (k, width)))
            out.append((float(low), float(np.nextafter(high, np.float32(-np.inf))), "k %d w %d high-" % (k, width)))
    out.append((0.25, -0.25, "low > high"))
    out.append((-0.5, 0.5, "whole circle"))
    return out


# through a bank: (samprate, L, M, D)
BANK_GEOMETRIES = (
    (192000, 512, 513, 4),       # N_dec = 256, bins 187.5 Hz apart
    (240000, 4800, 4801, 5),     # N = 9600, N_dec = 1920 = 2^7 3 5, bins 25 Hz apart
    (192000, 1024, 3073, 8),     # N_dec = 512, M_dec = 385 = 3 L_dec + 1: the pre-detection and the audio design rewrite taps
)


def bank_plan(samprate, L, M, D):
    """The channels of one bank geometry: FM, linear (ISB: the two-sideband scaling of REAL-type outputs) and AM, edges in Hz
    on bins of N_dec (multiples of the bin spacing) and off them, and the edges and beta each is retuned to afterwards."""
    spacing = samprate / (L + M - 1)                  # = dsamprate / N_dec
    on = lambda k: k * spacing                        # noqa: E731
    return [
        dict(demod="fm", low=on(-27), high=on(27), kaiser_beta=3.0, then=(on(-12), on(40), 1.0)),
        dict(demod="fm", low=-5100.0, high=4900.0, kaiser_beta=0.0, then=(-3333.0, on(16), 5.0)),
        dict(demod="linear", isb=1, low=on(-16), high=on(16), kaiser_beta=3.0, then=(on(1), on(15), 5.0)),
        dict(demod="linear", low=110.0, high=2900.0, kaiser_beta=3.0, then=(on(-15), -140.0, 1.0)),
        dict(demod="am", low=on(-24), high=on(24), kaiser_beta=3.0, then=(-4321.0, 4321.0, 1.0)),
    ]


def bank_batch_plan(samprate, L, M, D):
    """70 channels with 70 distinct edge pairs, and 70 more to retune them to (past one wave of design jobs)"""
    spacing = samprate / (L + M - 1)
    plan = []
    for i in range(70):
        demod = ("fm", "linear", "am")[i % 3]
        low, high = -(i + 2) * spacing * (1.0 if i % 2 else 1.013), (i % 31 + 3) * spacing * (1.0 if i % 4 < 2 else 0.991)
        plan.append(dict(demod=demod, isb=int(demod == "linear" and i % 2 == 1), flat=int(demod == "fm" and i % 6 == 3), low=low,
                         high=high, kaiser_beta=3.0, then=(-(i % 29 + 2.5) * spacing, (i + 3) * spacing, 1.0 if i % 2 else 5.0)))
    assert len({(p["low"], p["high"]) for p in plan}) == 70 and len({p["then"][:2] for p in plan}) == 70
    return plan


def retuned(p):
    """The channel after its set_filter"""
    return dict(p, low=p["then"][0], high=p["then"][1], kaiser_beta=p["then"][2])


def bank_model(geom, p, runtime):
    """-> (response, noise gain) of channel p of a bank of geometry geom: at start-up, or after its set_filter"""
    samprate, L, M, D = geom
    N, L_dec, M_dec, _ = band_geometry(L, M, D)
    now = retuned(p) if runtime else p
    lo, hi = normalised_edges(now, samprate, D, runtime)
    return set_filter(N, L_dec, M_dec, float(lo), float(hi), now["kaiser_beta"], two_sided(p))


def normalised_edges(p, samprate, D, runtime):
    """The edges set_filter is given, in cycles per output sample, in float as the demodulators form them: fm.c:35 low /
    dsamprate at start-up; am.c:41, linear.c:81 and every change made while running (display.c:161-177) samptime * low"""
    low, high = np.float32(p["low"]), np.float32(p["high"])
    if p["demod"] == "fm" and not runtime:
        dsamprate = np.float32(samprate) / np.float32(D)
        return low / dsamprate, high / dsamprate
    samptime = np.float32(D) / np.float32(samprate)
    return samptime * low, samptime * high


def two_sided(p):
    return p["demod"] == "linear" and bool(p.get("isb", 0))


@functools.lru_cache(maxsize=None)
def window_target(L, M, real):
    """The random target of a window case: fixed seed per shape; the REAL one carries imaginary parts in DC and Nyquist"""
    N = L + M - 1
    rng = np.random.default_rng(1000 * L + M + (500000 if real else 0))
    n = N // 2 + 1 if real else N
    r = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def window_model(L, M, beta, real):
    f = window_rfilter if real else window_filter
    r = f(L, M, window_target(L, M, real), beta)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def band_model(L, M, D, sidebands, low, high, beta=BAND_BETA):
    """set_filter of a slave at decimate D on an (L, M) master; sidebands 2: REAL and CROSS_CONJ outputs"""
    N, L_dec, M_dec, _ = band_geometry(L, M, D)
    r, ng = set_filter(N, L_dec, M_dec, low, high, beta, sidebands == 2)
    r.setflags(write=False)
    return r, ng


AUDIO_BETA = (3.0, 0.0)                               # the Kaiser betas of the FM channels of bank_plan


@functools.lru_cache(maxsize=None)
def audio_model(samprate, L, M, D, beta):
    r = audio_response(L // D, (M - 1) // D + 1, np.float32(samprate) / np.float32(D), beta)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def kaiser_model(M, beta):
    w = kaiser(M, beta)
    w.setflags(write=False)
    return w
