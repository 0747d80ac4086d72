"""NCO: the oracle restatement (oracle/kq_osc.c) against the reference itself.

oracle/_ref/libref_osc.so is the reference's osc.c + dsp.c compiled unmodified (oracle/Makefile), so
these tests PIN the restatement.  tests/golden/osc_*.npz hold sequences generated from that build
(tests/golden/make_golden.py) for boxes where neither the reference tree nor _ref is present; tests/golden/ref_pins.npz
holds that build's answers to the exact inputs of the tests below, which use them where _ref is not built.
"""
import ctypes as C
import os

import numpy as np
import pytest

import kq_oracle as ko

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PINS = os.path.join(GOLD, "ref_pins.npz")
TOL = 2e-11   # double recurrences compiled with different FP contraction flags
# Recorded sequences: each phasor's angle in units of 2^-PIN_BITS cycle and its modulus - 1 in units of 2^-PIN_BITS, kept as
# exact integer second / first differences (tests/golden/make_golden.py checks the decoded sequence is within PIN_ERR)
PIN_BITS = 50
PIN_ERR = 1e-14


def _run_oracle(script, n):
    L = ko.lib()
    o = ko.Osc()
    out = np.zeros((n, 2))
    for i in range(n):
        if i in script:
            f, r = script[i]
            L.kqo_set_osc(C.byref(o), f, r)
        z = L.kqo_step_osc(C.byref(o))
        out[i] = (z.re, z.im)
    return out, o.steps


def decode_pinned(d2, dm):
    """-> [n, 2] phasors from the recorded integer differences (the sums wrap modulo 2^64, a multiple of 2^PIN_BITS)"""
    one = np.int64(1) << PIN_BITS
    k = np.cumsum(np.cumsum(d2, dtype=np.int64), dtype=np.int64) & (one - 1)
    th = 2 * np.pi * (k.astype(np.float64) / float(one))
    m = 1.0 + np.cumsum(dm, dtype=np.int64).astype(np.float64) / float(one)
    return np.stack([m * np.cos(th), m * np.sin(th)], 1)


def _run_ref(script, n):
    R = ko.ref_osc_lib()
    o = ko.RefOsc()
    out = np.zeros((n, 2))
    for i in range(n):
        if i in script:
            f, r = script[i]
            R.set_osc(C.byref(o), f, r)
        z = R.step_osc(C.byref(o))
        out[i] = (z.re, z.im)
    return out, o.steps


SCRIPTS = {
    "fixed": ({0: (0.0123456789, 0.0)}, 40000),                       # > 2 renormalisation periods (osc.c:11)
    "sweep": ({0: (-0.31, 3.5e-10)}, 40000),
    "frozen": ({0: (0.0, 1e-9)}, 300),                                # freq == 0 never advances (osc.c:43)
    "retune": ({0: (0.1, 0.0), 5000: (-0.2000001, 0.0), 9000: (0.0, 0.0), 9500: (0.05, 1e-9)}, 20000),
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_oracle_osc_matches_reference_build(name):
    script, n = SCRIPTS[name]
    a, sa = _run_oracle(script, n)
    if ko.ref_osc_lib() is not None:
        b, sb = _run_ref(script, n)
        tol = TOL
    else:                                   # the same build's sequence, recorded to within PIN_ERR (tests/golden/make_golden.py)
        g = np.load(PINS)
        b, sb = decode_pinned(g["osc_%s_d2" % name], g["osc_%s_dm" % name]), int(g["osc_%s_steps" % name])
        tol = TOL - PIN_ERR
    assert sa == sb
    assert np.abs(a - b).max() < tol


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_oracle_osc_matches_golden(name):
    script, n = SCRIPTS[name]
    g = np.load(os.path.join(GOLD, "osc_%s.npz" % name))
    a, steps = _run_oracle(script, n)
    assert steps == int(g["steps"])
    idx = g["index"]
    assert np.abs(a[idx] - g["phasor"]).max() < TOL


def test_closed_form_matches_recurrence():
    """phase(n) = f n + r n (n-1)/2 (what the GPU evaluates) against the stepped reference phasor."""
    script, n = SCRIPTS["sweep"]
    a, _ = _run_oracle(script, n)
    f, r = script[0]
    k = np.arange(n, dtype=np.float64)
    ph = f * k + r * (0.5 * k * (k - 1.0))
    z = np.exp(2j * np.pi * (ph - np.rint(ph)))
    assert np.abs(a[:, 0] + 1j * a[:, 1] - z).max() < 1e-9


PHASOR_INIT_CASES = ((1.0, 0.0), (0.0, 0.0), (0.9, 0.3), (0.6, 0.6), (float("nan"), 0.0), (0.0, float("nan")))


def test_is_phasor_init():
    R, L = ko.ref_osc_lib(), ko.lib()
    L.kqo_is_phasor_init.argtypes = [ko._Cplx]
    recorded = np.load(PINS)["is_phasor_init"] if R is None else None
    for i, (re, im) in enumerate(PHASOR_INIT_CASES):
        z = ko._Cplx(re, im)
        want = R.is_phasor_init(z) if R is not None else int(recorded[i])
        assert want == L.kqo_is_phasor_init(z)
