"""The float64 model of the response design (tests/design_model.py) against the oracle, and against its own mutants.

Two things are established here, on the CPU, over the case tables that tests/test_gpu_design.py runs on the device:
* the oracle's float32 restatement of make_kaiser / window_filter / window_rfilter / set_filter / the FM audio design stays
  within the BASELINE recorded in design_model.py of the float64 model (the device's bar is 4 x that baseline);
* every case designated sensitive differs from its mutant -- the rotation out of place, a bin more at a band edge, the wrong
  Kaiser denominator, DC / Nyquist imaginary parts carried along -- by at least 10 bars: the device test would fail on it.
"""
import ctypes as C

import numpy as np
import pytest

import design_model as dm
import kq_oracle as ko
from common import oracle_cfg
from test_oracle_filter import _FilterOut as OFilterOut, _as


# ---- the oracle's side (also used by the device tests) --------------------------------------------------------------------
def oracle_window(L, M, beta, real):
    r = np.array(dm.window_target(L, M, real))
    f = ko.lib().kqo_window_rfilter if real else ko.lib().kqo_window_filter
    assert f(L, M, r.ctypes.data, beta) == 0
    return r


class OracleSlave:
    """An oracle slave at decimate D on a COMPLEX (L, M) master: set_filter -> (response, noise gain)"""

    def __init__(self, L, M, D, out_type):
        self.O = ko.lib()
        self.n_dec = (L + M - 1) // D
        self.m = self.O.kqo_create_filter_input(L, M, ko.KQO_COMPLEX)
        self.s = self.O.kqo_create_filter_output(self.m, None, D, out_type)
        assert self.m and self.s

    def set_filter(self, low, high, beta):
        rc = self.O.kqo_set_filter(self.s, low, high, beta)
        so = C.cast(self.s, C.POINTER(OFilterOut)).contents
        return rc, _as(so.response, self.n_dec, np.complex64).copy(), so.noise_gain

    def close(self):
        self.O.kqo_delete_filter_output(self.s)
        self.O.kqo_delete_filter_input(self.m)


def oracle_audio(samprate, L, M, D, beta):
    ch = ko.Channel(ko.make_cfg(samprate=samprate, L=L, M=M, D=D, demod_type=ko.KQO_FM, kaiser_beta=beta))
    r = ch.audio_response()
    ch.close()
    return r


def window_family(real, beta):
    return ("window_rfilter" if real else "window_filter") + ("_b9" if beta > 3.0 else "")


def window_cases(real):
    return [(L, M, b) for (L, M) in dm.WINDOW_SHAPES for b in dm.WINDOW_BETA] + [(L, M, 9.0) for (L, M) in dm.WINDOW_B9_SHAPES]


# ---- baselines: the oracle against the model --------------------------------------------------------------------------------
def measure_kaiser():
    worst = 0.0
    for M in dm.KAISER_M:
        for beta in dm.KAISER_BETA:
            worst = max(worst, float(np.abs(ko.make_kaiser(M, beta) - dm.kaiser_model(M, beta)).max()))
    return {"kaiser": worst}


def measure_windows(real):
    worst = {}
    for L, M, beta in window_cases(real):
        fam = window_family(real, beta)
        worst[fam] = max(worst.get(fam, 0.0), dm.rel_peak(oracle_window(L, M, beta, real), dm.window_model(L, M, beta, real)))
    return worst


def measure_band(L, M, D):
    worst = {"band": 0.0, "noise_gain": 0.0}
    n_dec = (L + M - 1) // D
    for out_type in dm.BAND_OUT_TYPES:
        s = OracleSlave(L, M, D, out_type)
        for low, high, what in dm.band_edges(n_dec):
            rc, r, ng = s.set_filter(low, high, dm.BAND_BETA)
            assert rc == 0
            want, want_ng = dm.band_model(L, M, D, 1 if out_type == dm.OUT_COMPLEX else 2, low, high)
            if not np.any(want):
                assert not np.any(r) and ng == 0, (out_type, what)      # an empty band: transforms of zeros are zeros
                continue
            worst["band"] = max(worst["band"], dm.rel_peak(r, want))
            worst["noise_gain"] = max(worst["noise_gain"], abs(ng - want_ng) / want_ng)
        s.close()
    return worst


def measure_audio():
    worst = 0.0
    for fs, L, M, D in dm.BANK_GEOMETRIES:
        for beta in dm.AUDIO_BETA:
            worst = max(worst, dm.rel_peak(oracle_audio(fs, L, M, D, beta), dm.audio_model(fs, L, M, D, beta)))
    return {"audio": worst}


def oracle_channel(geom, p, runtime):
    """The oracle's channel p of a bank of geometry geom: at start-up, or after its set_filter"""
    fs, L, M, D = geom
    ch = ko.Channel(oracle_cfg(p, fs, L, M, D))
    if runtime:
        ch.set_filter(*p["then"])
    return ch


def measure_bank():
    worst = 0.0
    for geom, plan in [(g, dm.bank_plan(*g)) for g in dm.BANK_GEOMETRIES] + [(dm.BANK_GEOMETRIES[0], dm.bank_batch_plan(*dm.BANK_GEOMETRIES[0]))]:
        for p in plan:
            for runtime in (False, True):
                want, want_ng = dm.bank_model(geom, p, runtime)
                assert np.count_nonzero(np.abs(want) > 0.5 * np.abs(want).max()) >= 2, (geom, p)
                ch = oracle_channel(geom, p, runtime)
                worst = max(worst, dm.rel_peak(ch.response(), want))
                assert abs(ch.noise_gain() - want_ng) / want_ng <= dm.BASELINE["noise_gain"], (geom, p)
                ch.close()
    return {"band_bank": worst}


def _check(worst):
    for fam, w in worst.items():
        print("%-18s oracle vs float64 %.3g   baseline %.3g   device bar %.3g" % (fam, w, dm.BASELINE[fam], dm.BAR[fam]))
    for fam, w in worst.items():
        assert w <= dm.BASELINE[fam], (fam, w)
        assert w >= dm.BASELINE[fam] / 4, ("the recorded baseline is stale: far above what the oracle does", fam, w)


def test_kaiser_oracle_within_baseline():
    _check(measure_kaiser())
    for M in dm.KAISER_M:
        for beta in dm.KAISER_BETA:
            w = dm.kaiser_model(M, beta)
            assert np.array_equal(w, w[::-1])
            if M % 2:
                assert w[M // 2] == 1.0
            if beta == 0:
                assert np.all(w == 1.0)


@pytest.mark.parametrize("real", [False, True])
def test_window_oracle_within_baseline(real):
    _check(measure_windows(real))


def test_band_oracle_within_baseline():
    worst = {"band": 0.0, "noise_gain": 0.0}
    for g in dm.BAND_GEOMETRIES:
        w = measure_band(*g)
        print(g, w)
        worst = {k: max(worst[k], w[k]) for k in worst}
    _check(worst)


def test_bank_oracle_within_baseline():
    _check(measure_bank())


def test_audio_oracle_within_baseline():
    _check(measure_audio())


def test_band_cases_are_what_they_say():
    """Edges exactly on a bin include it; one float inside, the edge bin drops out; low > high is empty; the whole circle."""
    for L, M, D in dm.BAND_GEOMETRIES:
        N, L_dec, M_dec, n_dec = dm.band_geometry(L, M, D)
        k = dm.signed_bins(n_dec)
        count = {}
        for low, high, what in dm.band_edges(n_dec):
            t = dm.band_target(N, L_dec, M_dec, low, high, False)
            count[what] = int(np.count_nonzero(t))
            if what.startswith("k ") and what.endswith(("w 0", "w 3")):
                k0, w = int(what.split()[1]), int(what.split()[3])
                assert np.array_equal(np.sort(k[t != 0]), np.arange(k0, min(k0 + w, n_dec // 2) + 1)), (L, M, D, what)
        for what, c in count.items():
            if what.endswith("low+"):
                assert c == count[what[:-5]] - 1, (L, M, D, what)
            if what.endswith("high-"):
                base = count[what[:-6]]
                k0, w = int(what.split()[1]), int(what.split()[3])
                assert c == (base - 1 if k0 + w <= n_dec // 2 else base), (L, M, D, what)
        assert count["low > high"] == 0 and count["whole circle"] == n_dec


# ---- sensitivity: the model against its mutants ---------------------------------------------------------------------------
def _bars(diff, family):
    return diff / dm.BAR[family]


def test_kaiser_denominator_is_seen():
    for M, beta in dm.KAISER_SENSITIVE:
        d = float(np.abs(dm.kaiser(M, beta, denom=M) - dm.kaiser_model(M, beta)).max())
        assert _bars(d, "kaiser") >= dm.SENSITIVITY_FACTOR, (M, beta, d)
    # ... and through a design, at even M
    L, M = 511, 514
    got = dm.window_filter(L, M, dm.window_target(L, M, False), 3.0, window=dm.kaiser(M, 3.0, denom=M))
    assert _bars(dm.rel_peak(got, dm.window_model(L, M, 3.0, False)), "window_filter") >= dm.SENSITIVITY_FACTOR


@pytest.mark.parametrize("real", [False, True])
def test_in_place_rule_is_seen(real):
    fam = "window_rfilter" if real else "window_filter"
    f = dm.window_rfilter if real else dm.window_filter
    for L, M in dm.WINDOW_SHAPES:
        assert (dm.rewritten_taps(L, M) > 0) == ((L, M) in dm.INPLACE_SHAPES), (L, M)
    assert dm.rewritten_taps(65, 128) == 0 and dm.rewritten_taps(64, 129) == 1
    for L, M, beta in (dm.INPLACE_SENSITIVE_REAL if real else dm.INPLACE_SENSITIVE):
        d = dm.rel_peak(f(L, M, dm.window_target(L, M, real), beta, in_place=False), dm.window_model(L, M, beta, real))
        print(fam, L, M, beta, "out of place differs by %.3g = %.0f bars" % (d, _bars(d, fam)))
        assert _bars(d, fam) >= dm.SENSITIVITY_FACTOR, (L, M, beta, d)
    for L, M in dm.WINDOW_B9_SHAPES:
        assert dm.rewritten_taps(L, M) == 0


def test_dc_and_nyquist_imaginary_parts_are_seen():
    for L, M in dm.WINDOW_SHAPES:
        for beta in dm.WINDOW_BETA:
            d = dm.rel_peak(dm.window_rfilter(L, M, dm.window_target(L, M, True), beta, keep_dc_imag=True),
                            dm.window_model(L, M, beta, True))
            assert _bars(d, "window_rfilter") >= dm.SENSITIVITY_FACTOR, (L, M, beta, d)


def test_a_flipped_bin_is_seen():
    """One bin more at either edge of every band of the table that has a bin there (the mutant of an empty band is one bin
    against nothing: the device test demands exact zeros there)."""
    least = np.inf
    for L, M, D in dm.BAND_GEOMETRIES:
        N, L_dec, M_dec, n_dec = dm.band_geometry(L, M, D)
        for low, high, what in dm.band_edges(n_dec):
            want, _ = dm.band_model(L, M, D, 1, low, high)
            base = dm.band_target(N, L_dec, M_dec, low, high, False)
            for extra in (+1, -1):
                t = dm.band_target(N, L_dec, M_dec, low, high, False, extra_bin=extra)
                if np.array_equal(t, base):
                    assert what == "whole circle" or "k %d " % (n_dec // 2) in what or "k %d " % (-n_dec // 2 + 1) in what or \
                        (extra > 0 and int(what.split()[1]) + int(what.split()[3]) >= n_dec // 2), (L, M, D, what, extra)
                    continue
                got = dm.window_filter(L_dec, M_dec, t, dm.BAND_BETA)
                if not np.any(want):
                    assert np.abs(got).max() > 1e-2 / N
                    continue
                d = dm.rel_peak(got, want)
                least = min(least, d)
                assert _bars(d, "band") >= dm.SENSITIVITY_FACTOR, (L, M, D, what, extra, d)
    print("a flipped bin: at least %.3g of the peak = %.0f bars" % (least, _bars(least, "band")))


def test_in_place_rule_is_seen_in_bands_and_audio():
    """M_dec = 385 on L_dec = 128: the long geometry's band designs and its FM audio design rewrite taps"""
    L, M, D = dm.BAND_GEOMETRIES[-1]
    N, L_dec, M_dec, n_dec = dm.band_geometry(L, M, D)
    assert dm.rewritten_taps(L_dec, M_dec) > 0
    for low, high, what in dm.band_edges(n_dec):
        want, _ = dm.band_model(L, M, D, 1, low, high)
        if np.any(want) and what != "whole circle":       # (all bins alike: a single tap, which no rotation rewrites)
            got, _ = dm.set_filter(N, L_dec, M_dec, low, high, dm.BAND_BETA, False, in_place=False)
            assert _bars(dm.rel_peak(got, want), "band") >= dm.SENSITIVITY_FACTOR, what
    fs, L, M, D = dm.BANK_GEOMETRIES[-1]
    assert dm.rewritten_taps(L // D, (M - 1) // D + 1) > 0
    for beta in dm.AUDIO_BETA:
        got = dm.audio_response(L // D, (M - 1) // D + 1, np.float32(fs) / np.float32(D), beta, in_place=False)
        d = dm.rel_peak(got, dm.audio_model(fs, L, M, D, beta))
        print("audio response, beta", beta, "out of place differs by %.3g = %.0f bars" % (d, _bars(d, "audio")))
        assert _bars(d, "audio") >= dm.SENSITIVITY_FACTOR, (beta, d)
