"""Argument checks of the spectrum bank (kq_spec_*): refused with -1 / NULL and a reason that names the function and the
field before any HIP call, so they hold without a GPU (kq_spec_create touches no device)."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.spectrum import SpecConfig, SpecInfo, _bind, spec_params

FS = 10000000


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _cfg(**kw):
    c = dict(device=0, samprate=FS, gain_factor=1.0, max_specs=8, max_samples=1 << 16, max_rows=4, stream=None)
    c.update(kw)
    return SpecConfig(*c.values())


@pytest.fixture
def bank(lib):
    h = lib.kq_spec_create(C.byref(_cfg()))
    assert h, lib.kq_last_error()
    yield h
    assert lib.kq_spec_destroy(h) == 0


def test_null_config_refused(lib):
    assert lib.kq_spec_create(None) is None
    assert lib.kq_last_error() == b"kq_spec_create: null config"


@pytest.mark.parametrize("kw,why", [
    (dict(samprate=0), b"samprate"),
    (dict(max_specs=0), b"max_specs"),
    (dict(max_specs=4097), b"max_specs"),
    (dict(max_samples=0), b"max_samples"),
    (dict(max_rows=0), b"max_rows"),
    (dict(gain_factor=float("nan")), b"gain_factor"),
])
def test_bad_config_refused(lib, kw, why):
    assert lib.kq_spec_create(C.byref(_cfg(**kw))) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_spec_create") and why in msg, msg


@pytest.mark.parametrize("kw,why", [
    (dict(fft_size=11 * 128), b"fft_size 1408"),            # prime factor 11
    (dict(fft_size=16384 + 2, bins=1024), b"fft_size"),     # past the limit
    (dict(fft_size=32768, bins=1024), b"fft_size"),
    (dict(fft_size=1001, bins=1000), b"fft_size 1001"),     # odd
    (dict(fft_size=8, bins=8), b"fft_size 8"),              # below 16
    (dict(fft_size=1024, bins=1023), b"bins 1023"),         # odd
    (dict(fft_size=1024, bins=0), b"bins 0"),
    (dict(fft_size=1024, bins=1026), b"bins 1026"),         # > Nf at Dz 1
    (dict(fft_size=1024, bins=770, decimate=4), b"3 fft_size / 4"),
    (dict(fft_size=1024, hop=0), b"hop 0"),
    (dict(fft_size=1024, hop=1025), b"hop 1025"),
    (dict(fft_size=1024, average=0), b"average"),
    (dict(fft_size=1024, decimate=0), b"decimate 0"),
    (dict(fft_size=1024, decimate=257), b"decimate 257"),
    (dict(fft_size=1024, center=float("nan")), b"center"),
    (dict(fft_size=1024, sweep=float("inf")), b"sweep"),
    (dict(fft_size=1024, kaiser_beta=-1.0), b"kaiser_beta"),
])
def test_bad_params_refused(lib, bank, kw, why):
    p = spec_params(**kw)
    for h in (None, bank):   # checked before the bank is looked at
        assert lib.kq_spec_set(h, 0, C.byref(p)) == -1
        msg = lib.kq_last_error()
        assert msg.startswith(b"kq_spec_set: ") and why in msg, msg


def test_out_of_band_center_refused(lib, bank):
    for c in (FS / 2 + 1, -FS / 2 - 1, 1e12):
        assert lib.kq_spec_set(bank, 0, C.byref(spec_params(1024, center=c))) == -1
        assert b"out of band" in lib.kq_last_error()


def test_bad_slot_refused(lib, bank):
    p = spec_params(1024)
    assert lib.kq_spec_set(None, 4096, C.byref(p)) == -1
    assert b"slot 4096" in lib.kq_last_error()
    assert lib.kq_spec_set(bank, 8, C.byref(p)) == -1     # max_specs = 8
    assert b"slot 8 >= max_specs 8" in lib.kq_last_error()
    assert lib.kq_spec_set(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_spec_set: null params"
    for fn in (lib.kq_spec_remove,):
        assert fn(bank, 3) == -1
        assert b"slot 3 holds no analyzer" in lib.kq_last_error()
    rows = np.empty(16, np.float32)
    assert lib.kq_spec_pull(bank, 9, rows.ctypes.data, 1, None) == -1
    assert lib.kq_last_error().startswith(b"kq_spec_pull: slot 9")
    info = SpecInfo()
    assert lib.kq_spec_get_info(bank, 0, C.byref(info)) == -1
    assert lib.kq_last_error().startswith(b"kq_spec_get_info: slot 0")


def test_bad_process_refused(lib, bank):
    buf = np.zeros(16, np.complex64)
    for fmt in (3, -1):
        assert lib.kq_spec_process(bank, buf.ctypes.data, fmt, 16, 0) == -1
        assert b"format" in lib.kq_last_error()
    assert lib.kq_spec_process(bank, buf.ctypes.data, 0, (1 << 16) + 1, 0) == -1
    assert b"max_samples" in lib.kq_last_error()
    assert lib.kq_spec_process(bank, None, 0, 16, 0) == -1
    assert b"null iq" in lib.kq_last_error()
    assert lib.kq_spec_process(bank, None, 0, 0, 0) == 0       # nothing to do
    assert lib.kq_spec_process(None, buf.ctypes.data, 0, 16, 0) == -1
    assert lib.kq_last_error() == b"kq_spec_process: null bank"


def test_null_handles_refused(lib):
    for fn, args in ((lib.kq_spec_destroy, ()), (lib.kq_spec_sync, ()), (lib.kq_spec_reset, ()), (lib.kq_spec_remove, (0,))):
        assert fn(None, *args) == -1
        assert b"null bank" in lib.kq_last_error()
