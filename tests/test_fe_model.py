"""The definition of the raw A/D conditioning stage (tests/fe_model.py: exact) against the reference's literal loop,
its convergence where that can be derived, and the argument checks of kq_fe_create.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import fe_model as fm

F = np.float32
TRAJ = ("DC_i", "DC_q", "imbalance", "sinphi", "in_power", "gain_i", "gain_q", "secphi", "tanphi")


def margins(fmt, block, fs, dc_alpha, power_alpha, nblocks, seed):
    """exact against literal on one stream: per state variable max |difference| over the blocks relative to the
    variable's largest magnitude, and the largest output difference relative to the output's RMS."""
    raw = fm.make_raw(fmt, block * nblocks, seed)
    ye, _, se = fm.exact(raw, fmt, block, fs, dc_alpha, power_alpha)
    yl, sl = fm.literal(raw, fmt, block, fs, dc_alpha, power_alpha)
    assert len(se) == len(sl) == nblocks
    got = {}
    for k in TRAJ:
        a = np.array([s[k] for s in se], np.float64)
        b = np.array([s[k] for s in sl], np.float64)
        got[k] = float(np.abs(a - b).max() / np.abs(b).max())
    got["output"] = float(np.abs(ye - yl).max() / np.sqrt(np.mean(np.abs(yl.astype(np.complex128)) ** 2)))
    for k in ("samples", "blocks", "clips"):
        assert [s[k] for s in se] == [s[k] for s in sl]
    return got


# Measured: per quantity the largest value over seeds 1..4, as margins() reports it.  `literal` differs
# from `exact` only by the rounding of its own sequential float32 sums, a random walk over summation order and input, so
# the bound is 4 x the observed maximum, as the feature's issue sets it.  (in_power is one such sum over the block divided
# by its length, hence the largest; secphi is 1 + 1e-3 here and differs by one float step at most.)
CASES = {
    # name: (fmt, block, fs, dc_alpha, power_alpha, nblocks, observed maxima)
    "hackrf": (fm.S8, 131072, 12288000, 1e-7, 1.0, 40,
               dict(DC_i=5.1e-06, DC_q=6.7e-06, imbalance=6.7e-06, sinphi=1.8e-05, in_power=0.00018,
                    gain_i=1.8e-06, gain_q=1.7e-06, secphi=1.2e-07, tanphi=1.8e-05, output=3.5e-06)),
    "hackrf, 10x faster estimator": (fm.S8, 131072, 12288000, 1e-7, 0.1, 40,
               dict(DC_i=5.1e-06, DC_q=6.7e-06, imbalance=4.6e-05, sinphi=3.9e-05, in_power=0.00018,
                    gain_i=1.5e-05, gain_q=1.2e-05, secphi=1.2e-07, tanphi=3.9e-05, output=2.5e-05)),
    "funcube": (fm.S16, 4096, 192000, 1e-6, 1.0, 160,
               dict(DC_i=1.9e-06, DC_q=1.1e-06, imbalance=3.6e-07, sinphi=5.5e-07, in_power=2.1e-06,
                    gain_i=1.2e-07, gain_q=1.2e-07, secphi=1.2e-07, tanphi=6.4e-07, output=5.6e-07)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_against_literal(case):
    fmt, block, fs, dc_alpha, power_alpha, nblocks, observed = CASES[case]
    got = margins(fmt, block, fs, dc_alpha, power_alpha, nblocks, seed=5)   # a seed the bounds were not measured on
    print(case, {k: "%.3g" % v for k, v in got.items()})
    for k in TRAJ + ("output",):
        assert got[k] <= 4 * observed[k], (k, got[k], observed[k])


def _tone_raw(fmt, block, nblocks, g, phi, dc, amp=0.5, cycles=16):
    """noise-free tone, a whole number of cycles per block, Q gain g, phase error phi, offset dc; quantised"""
    t = np.arange(block * nblocks, dtype=np.float64)
    w = 2 * np.pi * cycles / block
    full = 32767 if fmt == fm.S16 else 127
    i = np.round((amp * np.cos(w * t) + dc[0]) * full)
    q = np.round((g * amp * np.sin(w * t + phi) + dc[1]) * full)
    return np.stack([i, q], axis=1).astype(np.int16 if fmt == fm.S16 else np.int8)


def test_convergence_is_geometric():
    """Every block of a noise-free tone with whole cycles per block has the same energy ratio and the same normalised
    dot product, so imbalance and sinphi approach them with the error shrinking by (1 - r) per block,
    r = block / (adc_samprate * power_alpha); DC approaches the mean with (1 - dc_alpha * block) per block.
    r = 0.25, K = 64 blocks: 0.75^64 = 1e-8 < 1e-6.  dc_alpha * block = 0.25 likewise."""
    fmt, block, K = fm.S16, 4096, 64
    g, phi, dc = 1.25, 0.1, (0.03, -0.02)
    r = 0.25
    fs, dc_alpha = block / r, r / block
    raw = _tone_raw(fmt, block, K, g, phi, dc)
    _, _, st = fm.exact(raw, fmt, block, fs, dc_alpha, 1.0)
    last = st[-1]
    assert (1 - r) ** K < 1e-6
    # The quantiser adds an error of at most half a step, 1.5e-5 of full scale, to every sample: uniform, nearly
    # uncorrelated with the tone, so the block energies (0.125 and 0.195 of full scale squared) move by about
    # step^2 / 12 = 8e-11 absolutely plus a cross term of order 2 * amp * 1.5e-5 / sqrt(block) = 2.4e-7: relative
    # 2e-6.  The DC estimate moves by at most 1.5e-5 / sqrt(block) = 2.4e-7 of full scale (mean of the rounding
    # errors), and the same again while DC is still converging inside the energies.  Float rounding of the stored
    # state is 6e-8 relative.  The bounds below are those sums, rounded up to one digit.
    assert abs(last["imbalance"] - 1 / g ** 2) <= 1e-5 / g ** 2
    # with DC removed, dotprod / block_energy of the balanced tone is sin(phi) exactly when the gains have converged
    assert abs(last["sinphi"] - np.sin(phi)) <= 1e-5
    assert abs(last["DC_i"] - dc[0]) <= 1e-6 and abs(last["DC_q"] - dc[1]) <= 1e-6
    # and the rate is the derived one: the error after k blocks against (1 - r)^k, while it is far above the floor
    imb = np.array([s["imbalance"] for s in st[:12]], np.float64)
    err = np.abs(imb - 1 / g ** 2)
    # DC converges at the same time, which perturbs the early ratios at second order: 10 % slack on the per-block factor
    ratio = err[1:] / err[:-1]
    assert np.all(np.abs(ratio[3:] - (1 - r)) < 0.1 * (1 - r)), ratio


@pytest.mark.parametrize("fmt", [fm.S8, fm.S16])
def test_exact_is_invariant_to_call_boundaries(fmt):
    block = 1000
    raw = fm.make_raw(fmt, 10 * block + 123, seed=9)
    y, s16, st = fm.exact(raw, fmt, block, 48000, 1e-4, 0.5)
    m = fm.Exact(fmt, block, 48000, 1e-4, 0.5)
    ys, ss, sts = [], [], []
    pos = 0
    for n in (1, 999, 1, 2500, 17, 3000, 10**9):
        a, b, c = m.process(raw[pos:pos + n])
        ys.append(a), ss.append(b), sts.extend(c)
        pos += n
    assert np.array_equal(np.concatenate(ys).view(np.uint32), y.view(np.uint32))
    assert np.array_equal(np.concatenate(ss), s16)
    assert len(sts) == len(st) == 10
    for a, b in zip(sts, st):
        for k in fm.STATUS_FIELDS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_minus_128_rule_and_clip_count():
    """hackrf.c:146-153: -128 counts a clip (I and Q separately) and is taken as -127."""
    block = 64
    raw = np.zeros((2 * block, 2), np.int8)
    raw[:, 0] = 5
    raw[3] = (-128, 7)
    raw[10] = (-128, -128)
    raw[block + 1] = (9, -128)
    same = raw.copy()
    same[same == -128] = -127
    y, _, st = fm.exact(raw, fm.S8, block, 1000.0, 1e-3)
    y2, _, st2 = fm.exact(same, fm.S8, block, 1000.0, 1e-3)
    assert [s["clips"] for s in st] == [3, 4] and [s["clips"] for s in st2] == [0, 0]
    assert np.array_equal(y, y2)
    assert y[3].real == F(-127) * fm.scale_of(fm.S8)
    for a, b in zip(st, st2):
        assert all(a[k] == b[k] for k in TRAJ)
    _, lit = fm.literal(raw, fm.S8, block, 1000, 1e-3)
    assert [s["clips"] for s in lit] == [3, 4]


@pytest.mark.parametrize("fmt", [fm.S8, fm.S16])
def test_all_zero_block_updates_only_dc(fmt):
    """hackrf.c:184 `if(block_energy > 0)`: a block that is all zero after DC removal leaves everything but DC alone."""
    block = 256
    m = fm.Exact(fmt, block, 4096.0, 1e-3)
    m.process(fm.make_raw(fmt, 4 * block, seed=2))   # some state to keep
    # zero DC estimate is needed for the block energy to be exactly zero: start a second model from reset for that
    z = fm.Exact(fmt, block, 4096.0, 1e-3)
    _, _, st = z.process(np.zeros((block, 2), np.int16 if fmt == fm.S16 else np.int8))
    init = fm._initial()
    assert all(st[0][k] == init[k] for k in TRAJ) and st[0]["blocks"] == 1 and st[0]["samples"] == block
    # with state: zeros in, DC decays towards zero, the energies are n * DC^2 > 0, so the estimates do move
    before = dict(m.st)
    _, _, st = m.process(np.zeros((block, 2), np.int16 if fmt == fm.S16 else np.int8))
    assert abs(st[0]["DC_i"]) < abs(before["DC_i"]) and st[0]["in_power"] > 0


def _lib():
    import ka9q_sdr_amd as kq
    from ka9q_sdr_amd import frontend
    kq.build_library()
    return frontend._bind(kq.load_library()), frontend


@pytest.mark.parametrize("kw,why", [
    (dict(format=2), b"format"), (dict(format=-1), b"format"),
    (dict(block=63), b"block"), (dict(block=(1 << 22) + 1), b"block"), (dict(block=0), b"block"),
    (dict(adc_samprate=0.0), b"positive"), (dict(adc_samprate=-1.0), b"positive"),
    (dict(dc_alpha=0.0), b"positive"), (dict(power_alpha=-2.0), b"positive"),
    (dict(max_samples=0), b"max_samples"),
])
def test_create_checks_its_arguments_before_any_device_is_asked_for(kw, why):
    """Refused with the reason, with or without a GPU in the box: device 99 does not exist anywhere, and the message is
    about the argument, not about the device."""
    lib, frontend = _lib()
    cfg = dict(device=99, format=frontend.KQ_FE_S8, block=4096, adc_samprate=1e6, dc_alpha=1e-7, power_alpha=1.0,
               max_samples=1 << 16, stream=None)
    cfg.update(kw)
    h = lib.kq_fe_create(C.byref(frontend.FeConfig(**cfg)))
    assert h is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_fe_create: ") and why in msg, msg


def test_create_refuses_null_and_exports_its_surface():
    lib, _ = _lib()
    assert lib.kq_fe_create(None) is None
    assert lib.kq_last_error() == b"kq_fe_create: null config"
    for n in ("kq_fe_create", "kq_fe_destroy", "kq_fe_reset", "kq_fe_sync", "kq_fe_stream", "kq_fe_process",
              "kq_fe_process_decim", "kq_fe_get_status"):
        assert hasattr(lib, n), n
