"""Argument checks of the RDS decoder bank (kq_rds_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_rds_create touches no device)."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.rds import GROUP_DTYPE, STATUS_DTYPE, RdsConfig, _bind, rds_params


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _cfg(**kw):
    c = dict(device=0, comp_rate=384000, decimate=16, L=2048, M=2049, kaiser_beta=3.0, max_slots=8, max_samples=1 << 14,
             stream=None)
    c.update(kw)
    return RdsConfig(*c.values())


@pytest.fixture
def bank(lib):
    h = lib.kq_rds_create(C.byref(_cfg()))
    assert h, lib.kq_last_error()
    yield h
    assert lib.kq_rds_destroy(h) == 0


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    names = {"kq_rds_create", "kq_rds_destroy", "kq_rds_set", "kq_rds_remove", "kq_rds_process", "kq_rds_sync",
             "kq_rds_reset", "kq_rds_max_groups", "kq_rds_pull_baseband"}
    assert names <= decl
    for n in sorted(names):
        assert hasattr(lib, n), n


def test_record_layouts():
    assert GROUP_DTYPE.itemsize == 16 and STATUS_DTYPE.itemsize == 24
    assert GROUP_DTYPE.fields["bit"][1] == 12 and GROUP_DTYPE.fields["ok"][1] == 8


def test_null_config_refused(lib):
    assert lib.kq_rds_create(None) is None
    assert lib.kq_last_error() == b"kq_rds_create: null config"


def test_good_configs_accepted(lib):
    for kw in (dict(), dict(comp_rate=128000, decimate=8, L=512, M=513),       # N = 1024, the smallest
               dict(comp_rate=128000, decimate=4, L=256, M=769),
               dict(comp_rate=240000, decimate=8, L=1000, M=1001),             # N = 2000 = 2^4 5^3, N / Dr = 250
               dict(comp_rate=384000, decimate=32, L=2048, M=2049),
               dict(comp_rate=384000, decimate=16, L=8192, M=8193, max_slots=4096)):
        h = lib.kq_rds_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_rds_destroy(h) == 0


@pytest.mark.parametrize("kw,why", [
    (dict(comp_rate=127999), b"comp_rate 127999"),                    # Fc >= 128 kHz
    (dict(decimate=0), b"decimate 0"),
    (dict(decimate=7), b"decimate 7 must divide comp_rate"),          # Dr | Fc
    (dict(decimate=64), b"at least 9500"),                            # Fr = 6000 < 9500
    (dict(L=2040, M=2057), b"must divide L 2040"),                    # Dr | L
    (dict(M=2041), b"M - 1 2040"),                                    # Dr | M - 1
    (dict(M=2050), b"M 2050 must be odd"),
    (dict(L=8192, M=8209), b"N = L + M - 1 = 16400"),                 # N > 16384
    (dict(decimate=8, L=1352, M=1353), b"N = L + M - 1 = 2704"),      # 2704 = 2^4 13^2
    (dict(L=2000, M=2001), b"is not whole"),                          # 57000 x 4000 / 384000 = 593.75: off the bins
    (dict(comp_rate=128000, decimate=8, L=600, M=601), b"is not whole"),   # 57000 x 1200 / 128000 = 534.375
    (dict(comp_rate=128000, decimate=4, L=768, M=257), b"three bit periods"),  # (M - 1) / Fc = 2 ms < 2.53 ms
    (dict(comp_rate=128000, decimate=4, L=512, M=513, kaiser_beta=10.0), b"transition band"),   # 59375 + 5015 > 64000
    (dict(kaiser_beta=float("nan")), b"kaiser_beta"),
    (dict(kaiser_beta=-1.0), b"kaiser_beta"),
    (dict(max_slots=0), b"max_slots 0"),
    (dict(max_slots=4097), b"max_slots 4097"),
    (dict(max_samples=0), b"max_samples 0"),
])
def test_bad_config_refused(lib, kw, why):
    assert lib.kq_rds_create(C.byref(_cfg(**kw))) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_rds_create: ") and why in msg, msg


@pytest.mark.parametrize("kw,why", [
    (dict(track_ms=0.0), b"track_ms"),
    (dict(track_ms=-5.0), b"track_ms"),
    (dict(track_ms=float("nan")), b"track_ms"),
    (dict(track_ms=float("inf")), b"track_ms"),
    (dict(lose_after=0), b"lose_after 0"),
    (dict(lose_after=-3), b"lose_after -3"),
])
def test_bad_params_refused(lib, bank, kw, why):
    p = rds_params(**kw)
    for h in (None, bank):   # checked before the bank is looked at
        assert lib.kq_rds_set(h, 0, C.byref(p)) == -1
        msg = lib.kq_last_error()
        assert msg.startswith(b"kq_rds_set: ") and why in msg, msg


def test_bad_slot_refused(lib, bank):
    p = rds_params()
    assert lib.kq_rds_set(None, 4096, C.byref(p)) == -1
    assert b"slot 4096" in lib.kq_last_error()
    assert lib.kq_rds_set(bank, 8, C.byref(p)) == -1     # max_slots = 8
    assert b"slot 8 >= max_slots 8" in lib.kq_last_error()
    assert lib.kq_rds_set(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_rds_set: null params"
    assert lib.kq_rds_set(None, 0, C.byref(p)) == -1
    assert lib.kq_last_error() == b"kq_rds_set: null bank"
    assert lib.kq_rds_remove(bank, 3) == -1
    assert b"slot 3 holds no decoder" in lib.kq_last_error()
    buf = np.zeros(16, np.float32)
    assert lib.kq_rds_pull_baseband(bank, 3, buf.ctypes.data, 8) == -1
    assert b"slot 3 holds no decoder" in lib.kq_last_error()
    assert lib.kq_rds_pull_baseband(bank, 9, buf.ctypes.data, 8) == -1
    assert lib.kq_rds_pull_baseband(bank, 0, None, 8) == -1
    assert lib.kq_last_error() == b"kq_rds_pull_baseband: null dst_re_im"


def test_max_groups(lib, bank):
    # ceil(nsamples 1187.5 / Fc) / 104 + 2 at Fc = 384000: 16384 samples are 50.67 bits
    assert lib.kq_rds_max_groups(bank, 0) == 2
    assert lib.kq_rds_max_groups(bank, 16384) == 2
    assert lib.kq_rds_max_groups(bank, 384000) == 1188 // 104 + 2 == 13
    assert lib.kq_rds_max_groups(None, 100) == 0
    assert lib.kq_last_error() == b"kq_rds_max_groups: null bank"


def test_bad_process_refused(lib, bank):
    buf = np.zeros(1 << 15, np.float32)
    out = np.zeros(1 << 12, np.uint32)
    o = out.ctypes.data
    assert lib.kq_rds_process(bank, buf.ctypes.data, 0, 4096, 4096, 5, 0, None, 0, None, None, 0) == -1   # 20480 > 16384
    assert b"max_samples" in lib.kq_last_error()
    assert lib.kq_rds_process(bank, buf.ctypes.data, 0, 100, 200, 2, 0, None, 0, None, None, 0) == -1
    assert b"row_stride 100 < block_len 200" in lib.kq_last_error()
    assert lib.kq_rds_process(bank, buf.ctypes.data, 0, 4096, 4096, 1, 0, o, 1, None, None, 0) == -1
    assert b"groups_stride 1 < kq_rds_max_groups = 2" in lib.kq_last_error()
    assert lib.kq_rds_process(bank, buf.ctypes.data, 0, 4096, 4096, 1, 0, None, 0, None, o, 1) == -1
    assert b"status_stride 1 < F = 2" in lib.kq_last_error()
    assert lib.kq_rds_process(bank, None, 0, 16, 16, 1, 0, None, 0, None, None, 0) == -1
    assert b"null comp" in lib.kq_last_error()
    assert lib.kq_rds_process(bank, None, 0, 0, 0, 0, 0, None, 0, None, None, 0) == 0       # nothing to do
    assert lib.kq_rds_process(None, buf.ctypes.data, 0, 16, 16, 1, 0, None, 0, None, None, 0) == -1
    assert lib.kq_last_error() == b"kq_rds_process: null bank"


def test_frames_counted_without_a_device(lib, bank):
    """with no slot set, process touches no device and still returns the frames each call completes"""
    buf = np.zeros(1 << 14, np.float32)
    got = [lib.kq_rds_process(bank, buf.ctypes.data, 0, n, n, 1, 0, None, 0, None, None, 0) for n in (1000, 1000, 5000, 16384)]
    assert got == [0, 0, 3, 8]     # 2000 -> 0, 7000 -> 3, 23384 -> 11 frames of 2048 in all
    assert lib.kq_rds_reset(bank) == 0
    assert lib.kq_rds_process(bank, buf.ctypes.data, 0, 2048, 2048, 1, 0, None, 0, None, None, 0) == 1


def test_null_handles_refused(lib):
    for fn, args in ((lib.kq_rds_destroy, ()), (lib.kq_rds_sync, ()), (lib.kq_rds_reset, ()), (lib.kq_rds_remove, (0,)),
                     (lib.kq_rds_pull_baseband, (0, None, 0))):
        assert fn(None, *args) == -1
        assert b"null bank" in lib.kq_last_error()
