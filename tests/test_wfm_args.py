"""Argument checks of the FM stereo decoder bank (kq_wfm_*): every limit is refused with -1 / NULL and a reason that names
the function and the field before any HIP call, so they hold without a GPU (kq_wfm_create touches no device)."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.wfm import WfmConfig, _bind, wfm_params


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _cfg(**kw):
    c = dict(device=0, comp_rate=384000, decimate=8, L=2048, M=2049, kaiser_beta=3.0, pilot_bw=1000.0, max_slots=8,
             max_samples=1 << 14, stream=None)
    c.update(kw)
    return WfmConfig(*c.values())


@pytest.fixture
def bank(lib):
    h = lib.kq_wfm_create(C.byref(_cfg()))
    assert h, lib.kq_last_error()
    yield h
    assert lib.kq_wfm_destroy(h) == 0


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    names = {"kq_wfm_create", "kq_wfm_destroy", "kq_wfm_set", "kq_wfm_remove", "kq_wfm_process", "kq_wfm_sync",
             "kq_wfm_reset"}
    assert names <= decl
    for n in sorted(names):
        assert hasattr(lib, n), n


def test_null_config_refused(lib):
    assert lib.kq_wfm_create(None) is None
    assert lib.kq_last_error() == b"kq_wfm_create: null config"


def test_good_configs_accepted(lib):
    for kw in (dict(), dict(comp_rate=128000, decimate=4, L=1024, M=1025, pilot_bw=500.0),
               dict(comp_rate=384000, decimate=8, L=8192, M=8193, max_slots=4096),
               dict(comp_rate=240000, decimate=5, L=1500, M=1501),          # N = 3000 = 2^3 3 5^3
               dict(comp_rate=384000, decimate=12, L=12 * 250, M=12 * 250 + 1),
               dict(comp_rate=384000, decimate=8, L=3000, M=2001)):           # N / decimate = 625, odd
        h = lib.kq_wfm_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_wfm_destroy(h) == 0


@pytest.mark.parametrize("kw,why", [
    (dict(comp_rate=127999), b"comp_rate 127999"),              # Fc >= 128 kHz
    (dict(decimate=13, L=13 * 160, M=13 * 160 + 1), b"output rate"),   # Fo = 29.5 kHz < 32 kHz
    (dict(decimate=0), b"decimate 0"),
    (dict(L=2044), b"must divide L 2044"),                     # Da | L
    (dict(M=2045), b"M - 1 2044"),                             # Da | M - 1 (2045 odd)
    (dict(M=2050), b"M 2050 must be odd"),
    (dict(L=8192, M=8201), b"N = L + M - 1 = 16392"),           # N > 16384
    (dict(L=1352, M=1353), b"N = L + M - 1 = 2704"),            # 2704 = 2^4 13^2
    (dict(L=2048, M=2049, decimate=1, comp_rate=384000, max_samples=1 << 14, pilot_bw=7000.0), b"transition band"),
    (dict(L=256, M=257), b"transition band"),                  # M too short: 15 kHz + 9.4 kHz > 18.5 kHz
    (dict(kaiser_beta=float("nan")), b"kaiser_beta"),
    (dict(kaiser_beta=-1.0), b"kaiser_beta"),
    (dict(pilot_bw=0.0), b"pilot_bw"),
    (dict(max_slots=0), b"max_slots 0"),
    (dict(max_slots=4097), b"max_slots 4097"),
    (dict(max_samples=0), b"max_samples 0"),
])
def test_bad_config_refused(lib, kw, why):
    assert lib.kq_wfm_create(C.byref(_cfg(**kw))) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_wfm_create: ") and why in msg, msg


@pytest.mark.parametrize("kw,why", [
    (dict(deviation_hz=0.0), b"deviation_hz"),
    (dict(deviation_hz=float("inf")), b"deviation_hz"),
    (dict(deemph_us=-1.0), b"deemph_us"),
    (dict(deemph_us=float("nan")), b"deemph_us"),
    (dict(pilot_on_db=float("nan")), b"pilot_on_db"),
    (dict(pilot_on_db=10.0, pilot_off_db=12.0), b"pilot_off_db must not exceed"),
    (dict(pilot_min_hz=-1.0), b"pilot_min_hz"),
    (dict(pilot_tol_hz=float("inf")), b"pilot_tol_hz"),
])
def test_bad_params_refused(lib, bank, kw, why):
    p = wfm_params(**kw)
    for h in (None, bank):   # checked before the bank is looked at
        assert lib.kq_wfm_set(h, 0, C.byref(p)) == -1
        msg = lib.kq_last_error()
        assert msg.startswith(b"kq_wfm_set: ") and why in msg, msg


def test_bad_slot_refused(lib, bank):
    p = wfm_params()
    assert lib.kq_wfm_set(None, 4096, C.byref(p)) == -1
    assert b"slot 4096" in lib.kq_last_error()
    assert lib.kq_wfm_set(bank, 8, C.byref(p)) == -1     # max_slots = 8
    assert b"slot 8 >= max_slots 8" in lib.kq_last_error()
    assert lib.kq_wfm_set(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_wfm_set: null params"
    assert lib.kq_wfm_remove(bank, 3) == -1
    assert b"slot 3 holds no decoder" in lib.kq_last_error()


def test_bad_process_refused(lib, bank):
    buf = np.zeros(1 << 15, np.float32)
    out = np.zeros(1 << 16, np.float32)
    assert lib.kq_wfm_process(bank, buf.ctypes.data, 0, 4096, 4096, 5, 0, None, 0, None, 0) == -1   # 20480 > 16384
    assert b"max_samples" in lib.kq_last_error()
    assert lib.kq_wfm_process(bank, buf.ctypes.data, 0, 100, 200, 2, 0, None, 0, None, 0) == -1
    assert b"row_stride 100 < block_len 200" in lib.kq_last_error()
    assert lib.kq_wfm_process(bank, buf.ctypes.data, 0, 4096, 4096, 1, 0, out.ctypes.data, 100, None, 0) == -1
    assert b"out_stride 100" in lib.kq_last_error()                    # 2 frames of 256 outputs need 1024
    assert lib.kq_wfm_process(bank, buf.ctypes.data, 0, 4096, 4096, 1, 0, None, 0, out.ctypes.data, 1) == -1
    assert b"status_stride 1 < F = 2" in lib.kq_last_error()
    assert lib.kq_wfm_process(bank, None, 0, 16, 16, 1, 0, None, 0, None, 0) == -1
    assert b"null comp" in lib.kq_last_error()
    assert lib.kq_wfm_process(bank, None, 0, 0, 0, 0, 0, None, 0, None, 0) == 0       # nothing to do
    assert lib.kq_wfm_process(None, buf.ctypes.data, 0, 16, 16, 1, 0, None, 0, None, 0) == -1
    assert lib.kq_last_error() == b"kq_wfm_process: null bank"


def test_frames_counted_without_a_device(lib, bank):
    """with no slot set, process touches no device and still returns the frames each call completes"""
    buf = np.zeros(1 << 14, np.float32)
    got = [lib.kq_wfm_process(bank, buf.ctypes.data, 0, n, n, 1, 0, None, 0, None, 0) for n in (1000, 1000, 5000, 16384)]
    assert got == [0, 0, 3, 8]     # 2000 -> 0, 7000 -> 3, 23384 -> 11 frames of 2048 in all
    assert lib.kq_wfm_reset(bank) == 0
    assert lib.kq_wfm_process(bank, buf.ctypes.data, 0, 2048, 2048, 1, 0, None, 0, None, 0) == 1


def test_null_handles_refused(lib):
    for fn, args in ((lib.kq_wfm_destroy, ()), (lib.kq_wfm_sync, ()), (lib.kq_wfm_reset, ()), (lib.kq_wfm_remove, (0,))):
        assert fn(None, *args) == -1
        assert b"null bank" in lib.kq_last_error()
