"""The response design kernels (kq_design.hip: k_design<REAL>, k_kaiser) bin by bin against the float64 model of the
reference's procedure (tests/design_model.py), and against the oracle at the tolerances the other tests use.

Every filter of the library comes out of these kernels, and a wrong response is silent: each block afterwards is filtered
"correctly" with the wrong filter, and audio at 1e-5 relative RMS does not see a flipped edge bin of a wide band or the
in-place rotation rule under a beta = 9 window.  So the responses themselves are compared here, over the case tables of
design_model.py, at the shapes where the kernel can go wrong: N = 2 and N = 16384 (the LDS limit), mixed radix, even M,
M <= 2, beta = 0, impulse responses of two blocks and more (the in-place rule, complex and REAL), band edges exactly on bins
and one float inside them, through all three ways in (the blocking batch, the on-stream batch of a bank, k_kaiser) and all
three target kinds (given, band, de-emphasis).

Bars: against the model, design_model.BAR of the case's family (4 x the oracle's own error against the model, measured on the
CPU by tests/test_design_model.py, which also shows each sensitive case to lie 10 bars from its mutant); against the oracle,
rtol 3e-7 for Kaiser taps, 1e-6 of the peak for window_filter / window_rfilter / set_filter responses, rtol 1e-5 for noise
gains, atol 2e-9 for a bank's responses.  Each test prints the worst device error of its families next to the bar.
"""
import ctypes as C

import numpy as np
import pytest

import design_model as dm
import ka9q_sdr_amd as kq
import kq_oracle as ko
from common import bank_cfg
from test_design_model import OracleSlave, oracle_channel, oracle_window, window_family
from test_gpu_compat import FilterIn, FilterOut
from test_oracle_filter import _as

pytestmark = pytest.mark.gpu

KAISER_ORACLE_RTOL = 3e-7
WINDOW_ORACLE_TOL = 1e-6        # of the oracle's peak
NOISE_GAIN_ORACLE_RTOL = 1e-5
BANK_ORACLE_ATOL = 2e-9

WORST = {}                      # family -> worst device error against the model so far in this run


def note(family, err):
    WORST[family] = max(WORST.get(family, 0.0), float(err))
    return float(err)


def report(*families):
    for f in families:
        if f in WORST:
            print("%-18s worst device error vs float64 %.3g   bar %.3g" % (f, WORST[f], dm.BAR[f]))


@pytest.fixture(scope="module")
def lib(gpu):
    L = kq.load_library()
    L.create_filter_input.restype = C.POINTER(FilterIn)
    L.create_filter_input.argtypes = [C.c_uint, C.c_uint, C.c_int]
    L.create_filter_output.restype = C.POINTER(FilterOut)
    L.create_filter_output.argtypes = [C.POINTER(FilterIn), C.c_void_p, C.c_uint, C.c_int]
    L.delete_filter_input.argtypes = [C.POINTER(FilterIn)]
    L.delete_filter_output.argtypes = [C.POINTER(FilterOut)]
    L.set_filter.argtypes = [C.POINTER(FilterOut), C.c_float, C.c_float, C.c_float]
    L.make_kaiser.argtypes = [C.c_void_p, C.c_uint, C.c_float]
    L.window_filter.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float]
    L.window_rfilter.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float]
    return L


# ---- k_kaiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", dm.KAISER_M)
def test_make_kaiser(lib, M):
    """M = 257 is past one 256-thread block of k_kaiser.  beta = 10 is one of the values at which float(pi) * beta, rounded
    twice, is one float away from the reference's double product rounded once (filter.c:342); taken the first way the taps were
    2e-6 relative from the oracle's, seven times the tolerance here."""
    for beta in dm.KAISER_BETA:
        w = np.full(M, np.nan, np.float32)
        assert lib.make_kaiser(w.ctypes.data, M, beta) == 0
        assert np.array_equal(w, w[::-1]), (M, beta)                       # bitwise symmetric (filter.c:348-351)
        if M % 2:
            assert w[M // 2] == 1.0, (M, beta)                             # filter.c:354-356
        if beta == 0:
            assert np.all(w == 1.0), M
        err = note("kaiser", np.abs(w - dm.kaiser_model(M, beta)).max())
        print("M", M, "beta", beta, "vs float64", err)
        assert err <= dm.BAR["kaiser"], (M, beta, err)
        np.testing.assert_allclose(w, ko.make_kaiser(M, beta), rtol=KAISER_ORACLE_RTOL, err_msg="M %d beta %g" % (M, beta))
    report("kaiser")


# ---- k_design, a given target: window_filter (complex taps) and window_rfilter (REAL) ---------------------------------------
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("L,M", dm.WINDOW_SHAPES)
def test_window_filter(lib, L, M, real):
    """Random complex targets (DC and Nyquist of the REAL ones carry imaginary parts, which c2r ignores); beta 0 and 3 on every
    shape, beta 9 on three shapes without rewritten taps.  No shape is refused: N = 2 and N = 16384 are inside the limits
    design_batch states (2 .. 16384)."""
    f = lib.window_rfilter if real else lib.window_filter
    betas = dm.WINDOW_BETA + ((9.0,) if (L, M) in dm.WINDOW_B9_SHAPES else ())
    for beta in betas:
        fam = window_family(real, beta)
        r = np.array(dm.window_target(L, M, real))
        assert f(L, M, r.ctypes.data, beta) == 0, (L, M, beta, kq.load_library().kq_last_error())
        err = note(fam, dm.rel_peak(r, dm.window_model(L, M, beta, real)))
        o = oracle_window(L, M, beta, real)
        err_o = np.abs(r - o).max() / np.abs(o).max()
        print(fam, (L, M), "beta", beta, "rewritten taps", dm.rewritten_taps(L, M), "vs float64 %.3g (bar %.3g)  vs oracle %.3g"
              % (err, dm.BAR[fam], err_o))
        assert err <= dm.BAR[fam], (L, M, beta, err)
        assert err_o < WINDOW_ORACLE_TOL, (L, M, beta, err_o)
    report(*sorted({window_family(real, b) for b in betas}))


# ---- k_design, a band: set_filter of the one-channel surface ------------------------------------------------------------------
@pytest.mark.parametrize("out_type", dm.BAND_OUT_TYPES, ids=["complex", "cross_conj", "real"])
@pytest.mark.parametrize("L,M,D", dm.BAND_GEOMETRIES)
def test_set_filter_bins(lib, L, M, D, out_type):
    """Edges exactly on bins, one float inside them (the edge bin drops out), low > high (all zero, noise gain 0, returns 0)
    and the whole circle: the response and the noise gain of every case of design_model.band_edges."""
    n_dec = (L + M - 1) // D
    m = lib.create_filter_input(L, M, 1)
    s = lib.create_filter_output(m, None, D, out_type)
    assert m and s
    o = OracleSlave(L, M, D, out_type)
    for low, high, what in dm.band_edges(n_dec):
        assert lib.set_filter(s, low, high, dm.BAND_BETA) == 0, what
        r = _as(s.contents.response, n_dec, np.complex64).copy()
        ng = float(s.contents.noise_gain)
        want, want_ng = dm.band_model(L, M, D, 1 if out_type == dm.OUT_COMPLEX else 2, low, high)
        if not np.any(want):
            assert not np.any(r) and ng == 0, what
            continue
        err, err_ng = dm.rel_peak(r, want), abs(ng - want_ng) / want_ng
        note("band", err)
        note("noise_gain", err_ng)
        assert err <= dm.BAR["band"], (what, err)
        assert err_ng <= dm.BAR["noise_gain"], (what, err_ng)
        rc, ro, ng_o = o.set_filter(low, high, dm.BAND_BETA)
        assert rc == 0
        assert np.abs(r - ro).max() / np.abs(ro).max() < WINDOW_ORACLE_TOL, what
        np.testing.assert_allclose(ng, ng_o, rtol=NOISE_GAIN_ORACLE_RTOL, err_msg=what)
    o.close()
    assert lib.delete_filter_output(s) == 0 and lib.delete_filter_input(m) == 0
    report("band", "noise_gain")


# ---- through a bank: the on-stream batch (design_launch) and the de-emphasis design -------------------------------------------
def _check_bank(bank, geom, plan, runtime, noise_gains=None, oracle_every=1):
    fs, L, M, D = geom
    for c, p in enumerate(plan):
        want, want_ng = dm.bank_model(geom, p, runtime)
        got = bank.response(c)
        err = note("band_bank", dm.rel_peak(got, want))
        if len(plan) < 10:
            print(geom, "ch", c, p["demod"], "retuned" if runtime else "start-up", "response vs float64 %.3g" % err)
        assert err <= dm.BAR["band_bank"], (geom, c, runtime, err)
        fm_audio = p["demod"] == "fm" and not p.get("flat", 0)
        if fm_audio:
            # designed once, in the demodulator's prologue (fm.c:54-66), with the beta of that moment: a later set_filter leaves it
            a = bank.audio_response(c)
            err_a = note("audio", dm.rel_peak(a, dm.audio_model(fs, L, M, D, p["kaiser_beta"])))
            assert err_a <= dm.BAR["audio"], (geom, c, err_a)
        if noise_gains is not None:
            err_ng = note("noise_gain", abs(noise_gains[c] - want_ng) / want_ng)
            assert err_ng <= dm.BAR["noise_gain"], (geom, c, err_ng)
        if c % oracle_every and c != len(plan) - 1:
            continue
        ch = oracle_channel(geom, p, runtime)
        np.testing.assert_allclose(got, ch.response(), rtol=0, atol=BANK_ORACLE_ATOL)
        if noise_gains is not None:
            np.testing.assert_allclose(noise_gains[c], ch.noise_gain(), rtol=NOISE_GAIN_ORACLE_RTOL)
        if fm_audio:
            ao = ch.audio_response()
            assert np.abs(a - ao).max() / np.abs(ao).max() < WINDOW_ORACLE_TOL, (geom, c)
        ch.close()


@pytest.mark.parametrize("geom", dm.BANK_GEOMETRIES, ids=["n1024_d4", "n9600_d5", "n4096_m3073_d8"])
def test_bank_designs_on_its_stream(gpu, geom):
    """Channels added one by one are designed by the launch on the bank's stream (design_launch with targets), which the
    one-channel surface never takes: FM (with its audio response, the REAL de-emphasis design), linear with both sidebands
    and AM, edges in Hz on bins of N_dec and off them; then set_filter on every channel with new edges and beta 1 and 5.  The
    responses are fetched without processing (kq_bank_get_response applies what is queued); on the first geometry one block
    is processed after the retune and the noise gains the launch left on the device are read from the block's status.
    On the third geometry M_dec = 385 on blocks of 128: the pre-detection and the audio design both rewrite taps."""
    fs, L, M, D = geom
    plan = dm.bank_plan(*geom)
    bank = kq.Bank(fs, L, M, D, len(plan), 1)
    for p in plan:
        bank.add_channel(bank_cfg(p))
    _check_bank(bank, geom, plan, runtime=False)
    for c, p in enumerate(plan):
        bank.set_filter(c, *p["then"])
    ngs = None
    if geom == dm.BANK_GEOMETRIES[0]:
        rng = np.random.default_rng(5)
        bank.push_iq((0.1 * (rng.standard_normal(L) + 1j * rng.standard_normal(L))).astype(np.complex64))
        assert bank.process() == 1
        ngs = [bank.status(c, 0)["noise_gain"] for c in range(len(plan))]
    _check_bank(bank, geom, plan, runtime=True, noise_gains=ngs)
    bank.close()
    report("band_bank", "noise_gain", "audio")


def test_bank_batch_of_70_distinct_filters(gpu):
    """70 channels with 70 distinct edge pairs in one add_channels call (the blocking batch, one launch per output type), then
    70 set_filter calls gathered into one launch on the stream: job indexing past one wave of jobs, each response against the
    model."""
    geom = dm.BANK_GEOMETRIES[0]
    fs, L, M, D = geom
    plan = dm.bank_batch_plan(*geom)
    bank = kq.Bank(fs, L, M, D, len(plan), 1)
    assert bank.add_channels([bank_cfg(p) for p in plan]) == list(range(70))
    _check_bank(bank, geom, plan, runtime=False, oracle_every=7)
    for c, p in enumerate(plan):
        bank.set_filter(c, *p["then"])
    _check_bank(bank, geom, plan, runtime=True, oracle_every=7)
    bank.close()
    report("band_bank", "audio")


def test_worst_device_errors_per_family():
    """The table of the run: every family's worst device error against the float64 model, next to its bar (run last)"""
    for fam in sorted(dm.BAR):
        print("%-18s worst device error vs float64 %-10s bar %.3g = %g x the oracle's %.3g"
              % (fam, "%.3g" % WORST[fam] if fam in WORST else "(not run)", dm.BAR[fam], dm.DEVICE_FACTOR, dm.BASELINE[fam]))
    for fam, w in WORST.items():
        assert w <= dm.BAR[fam], (fam, w)
