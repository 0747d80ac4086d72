"""What the float64 model of the FM stereo decoder (tests/wfm_model.py, the algorithm of kq_wfm_* in include/ka9q_hip.h)
itself reads on synthetic multiplexes: separation, de-emphasis, the pilot's frequency, mono without a pilot, and the
stereo flag's hysteresis."""
import numpy as np
import pytest

import wfm_model as wm

FC, DA, L, M = 192000, 4, 1024, 1025
FO = FC / DA


@pytest.fixture(scope="module")
def model():
    return wm.WfmModel(FC, DA, L, M)


def _t(n):
    return np.arange(n) / FC


@pytest.mark.parametrize("hz", [1000.0, 10000.0])
@pytest.mark.parametrize("side", ["L", "R"])
def test_separation(model, hz, side):
    n = 32 * L
    tone = np.sin(2 * np.pi * hz * _t(n))
    x = wm.multiplex(n, FC, tone if side == "L" else 0.0, tone if side == "R" else 0.0)
    out, st = model.decode(x, deemph_us=0)
    assert st["stereo"][2:].all()
    y = out[len(out) // 4:]
    amp = [wm.tone_amp(y[:, c], FO, hz) for c in (0, 1)]
    want, leak = (amp[0], amp[1]) if side == "L" else (amp[1], amp[0])
    assert abs(want - 1.0) < 1e-3                  # a full-scale channel reads 1.0
    assert 20 * np.log10(want / leak) >= 50.0


@pytest.mark.parametrize("tau", [75.0, 50.0])
def test_deemphasis(model, tau):
    n = 48 * L
    got = {}
    for hz in (100.0, 1000.0, 10000.0):
        x = wm.multiplex(n, FC, 0.5 * np.sin(2 * np.pi * hz * _t(n)), 0.5 * np.sin(2 * np.pi * hz * _t(n)), pilot=0.0)
        out, st = model.decode(x, deemph_us=tau)
        assert not st["stereo"].any()
        got[hz] = wm.tone_amp(out[len(out) // 4:, 0], FO, hz)
    for hz in (1000.0, 10000.0):
        want = 1 / abs(1 + 2j * np.pi * hz * tau * 1e-6) * abs(1 + 2j * np.pi * 100.0 * tau * 1e-6)
        assert abs(20 * np.log10(got[hz] / got[100.0] / want)) <= 0.1, (tau, hz)


def test_pilot_frequency(model):
    n = 16 * L
    x = wm.multiplex(n, FC, 0.3 * np.sin(2 * np.pi * 700 * _t(n)), 0.0, pilot_hz=19001.7)
    _, st = model.decode(x)
    assert np.all(np.abs(st["pilot_hz"][2:] - 19001.7) < 0.1)
    assert np.all(np.abs(st["pilot_dev_hz"][2:] - 7500.0) < 10.0)   # 0.1 of 75 kHz


@pytest.mark.parametrize("pilot", [0.0, 0.02])     # none, and 1.5 kHz of deviation: below pilot_min_hz 2000
def test_mono_without_pilot(model, pilot):
    n = 16 * L
    x = wm.multiplex(n, FC, 0.5 * np.sin(2 * np.pi * 1000 * _t(n)), 0.2 * np.sin(2 * np.pi * 3000 * _t(n)), pilot=pilot)
    out, st = model.decode(x)
    assert not st["stereo"].any()
    assert np.array_equal(out[:, 0], out[:, 1])


def test_hysteresis_across_a_fading_pilot(model):
    """noise of fixed level, the pilot fading down and back up: the flag holds on between off_db and on_db going down and
    holds off between them coming back"""
    n = 96 * L
    db = np.interp(np.arange(96), [0, 48, 96], [0.0, -40.0, 0.0])   # one level per frame, 0.83 dB steps
    env = 0.1 * np.repeat(10 ** (db / 20), L)
    rng = np.random.default_rng(3)
    x = wm.multiplex(n, FC, 0.0, 0.0, pilot=env) + 0.02 * rng.standard_normal(n)
    p = wm.params(pilot_on_db=20.0, pilot_off_db=10.0, pilot_min_hz=0.0, pilot_tol_hz=50.0)
    _, st = model.decode(x, **{k: v for k, v in p.items()})
    snr, on = st["pilot_snr_db"], st["stereo"]
    assert on.any() and not on.all()
    # every frame follows the rule from the one before
    prev = 0
    for f in range(len(on)):
        ok_f = abs(st["pilot_hz"][f] - 19000) <= 50
        want = (ok_f and snr[f] >= 10.0) if prev else (ok_f and snr[f] >= 20.0)
        assert on[f] == int(want), f
        prev = on[f]
    # frames between the thresholds take both values: which depends on where the flag came from
    mid = (snr >= 10.0) & (snr < 20.0)
    assert on[mid].any() and not on[mid].all()
    # force_mono pins the flag
    _, st2 = model.decode(x, **dict(p, force_mono=1))
    assert not st2["stereo"].any()
