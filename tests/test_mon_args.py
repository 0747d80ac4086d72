"""Argument checks of the monitor mixer bank (kq_mon_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU; create, set, adjust, remove and destroy touch no
device at all."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.monitor import KQ_MON_F32, KQ_MON_S16BE, MonConfig, STATUS_DTYPE, _bind, mon_params

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _cfg(**kw):
    c = dict(device=0, samprate=48000, max_sessions=16, max_buses=4, max_samples=1024, stream=None)
    c.update(kw)
    return MonConfig(*c.values())


@pytest.fixture
def bank(lib):
    h = lib.kq_mon_create(C.byref(_cfg()))
    assert h, lib.kq_last_error()
    yield h
    assert lib.kq_mon_destroy(h) == 0


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    names = {"kq_mon_create", "kq_mon_destroy", "kq_mon_set", "kq_mon_adjust", "kq_mon_remove", "kq_mon_process",
             "kq_mon_sync", "kq_mon_reset"}
    assert names <= decl
    for n in sorted(names):
        assert hasattr(lib, n), n


def test_status_record_is_20_bytes():
    assert STATUS_DTYPE.itemsize == 20
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    src = ('#include <stddef.h>\n#include "ka9q_hip.h"\n'
           '_Static_assert(sizeof(kq_mon_status) == 20, "size");\n'
           '_Static_assert(offsetof(kq_mon_status, clipped) == 8 && offsetof(kq_mon_status, active) == 16, "layout");\n'
           '_Static_assert(sizeof(kq_mon_params) == 24 && KQ_MON_F32 == 0 && KQ_MON_S16BE == 1, "params");\n'
           'int main(void) { return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        with open(p, "w") as f:
            f.write(src)
        r = subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(root, "include"), "-fsyntax-only", p], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
    assert C.sizeof(MonConfig) == 32 and (KQ_MON_F32, KQ_MON_S16BE) == (0, 1)


def test_null_config_refused(lib):
    assert lib.kq_mon_create(None) is None
    assert lib.kq_last_error() == b"kq_mon_create: null config"


def test_good_configs_accepted(lib):
    for kw in (dict(), dict(samprate=8000), dict(samprate=384000), dict(max_sessions=65536, max_buses=256),
               dict(max_sessions=1, max_buses=1, max_samples=1), dict(samprate=44100, max_samples=1 << 20)):
        h = lib.kq_mon_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_mon_destroy(h) == 0


@pytest.mark.parametrize("kw,why", [
    (dict(samprate=7999), b"samprate 7999"),
    (dict(samprate=384001), b"samprate 384001"),
    (dict(samprate=0), b"samprate 0"),
    (dict(max_sessions=0), b"max_sessions 0"),
    (dict(max_sessions=65537), b"max_sessions 65537"),
    (dict(max_buses=0), b"max_buses 0"),
    (dict(max_buses=257), b"max_buses 257"),
    (dict(max_samples=0), b"max_samples 0"),
])
def test_bad_config_refused(lib, kw, why):
    assert lib.kq_mon_create(C.byref(_cfg(**kw))) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_mon_create: ") and why in msg, msg


@pytest.mark.parametrize("kw,why", [
    (dict(channels=0), b"channels 0"),
    (dict(channels=3), b"channels 3"),
    (dict(gain=-0.5), b"gain"),
    (dict(gain=NAN), b"gain"),
    (dict(gain=INF), b"gain"),
    (dict(pan=1.0001), b"pan"),
    (dict(pan=-1.5), b"pan"),
    (dict(pan=NAN), b"pan"),
    (dict(pan=INF), b"pan"),
])
def test_bad_params_refused(lib, bank, kw, why):
    p = mon_params(**kw)
    for h in (None, bank):   # checked before the bank is looked at
        assert lib.kq_mon_set(h, 0, C.byref(p)) == -1
        msg = lib.kq_last_error()
        assert msg.startswith(b"kq_mon_set: ") and why in msg, msg


def test_bad_slot_and_bus_refused(lib, bank):
    p = mon_params()
    assert lib.kq_mon_set(None, 65536, C.byref(p)) == -1
    assert b"slot 65536" in lib.kq_last_error()
    assert lib.kq_mon_set(bank, 16, C.byref(p)) == -1     # max_sessions = 16
    assert lib.kq_last_error() == b"kq_mon_set: slot 16 >= max_sessions 16"
    assert lib.kq_mon_set(bank, 0, C.byref(mon_params(bus=4))) == -1     # max_buses = 4
    assert lib.kq_last_error() == b"kq_mon_set: bus 4 >= max_buses 4"
    assert lib.kq_mon_set(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_mon_set: null params"
    assert lib.kq_mon_set(None, 0, C.byref(p)) == -1
    assert lib.kq_last_error() == b"kq_mon_set: null bank"


def test_empty_slots_refused(lib, bank):
    assert lib.kq_mon_remove(bank, 3) == -1
    assert lib.kq_last_error() == b"kq_mon_remove: slot 3 holds no session"
    assert lib.kq_mon_adjust(bank, 3, 1.0, 0.0, 0) == -1
    assert lib.kq_last_error() == b"kq_mon_adjust: slot 3 holds no session"
    assert lib.kq_mon_adjust(bank, 16, 1.0, 0.0, 0) == -1
    assert b"kq_mon_adjust: slot 16" in lib.kq_last_error()
    assert lib.kq_mon_remove(bank, 99999) == -1
    assert b"kq_mon_remove: slot 99999" in lib.kq_last_error()


@pytest.mark.parametrize("gain,pan,why", [(-1.0, 0.0, b"gain"), (NAN, 0.0, b"gain"), (INF, 0.0, b"gain"), (1.0, 1.5, b"pan"),
                                          (1.0, NAN, b"pan"), (1.0, -INF, b"pan")])
def test_bad_adjust_refused(lib, bank, gain, pan, why):
    assert lib.kq_mon_set(bank, 2, C.byref(mon_params())) == 0
    assert lib.kq_mon_adjust(bank, 2, gain, pan, 0) == -1
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_mon_adjust: ") and why in msg, msg


def test_sessions_come_and_go_without_a_device(lib, bank):
    """set (also over an occupied slot, also at the limits of gain and pan), adjust, remove, reset and sync: host state only"""
    for slot, kw in ((0, dict()), (15, dict(source=70000, bus=3, channels=2, gain=0.0, pan=-1.0)),
                     (0, dict(channels=2, pan=1.0, muted=1)), (7, dict(gain=2.0, pan=0.25))):
        assert lib.kq_mon_set(bank, slot, C.byref(mon_params(**kw))) == 0, lib.kq_last_error()
    assert lib.kq_mon_adjust(bank, 7, 0.5, -1.0, 1) == 0
    assert lib.kq_mon_adjust(bank, 7, 0.0, 1.0, 0) == 0
    assert lib.kq_mon_remove(bank, 7) == 0
    assert lib.kq_mon_remove(bank, 7) == -1
    assert lib.kq_mon_adjust(bank, 7, 1.0, 0.0, 0) == -1
    assert lib.kq_mon_reset(bank) == 0
    assert lib.kq_mon_sync(bank) == 0
    assert lib.kq_mon_remove(bank, 0) == 0 and lib.kq_mon_remove(bank, 15) == 0


def test_bad_process_refused(lib, bank):
    buf = np.zeros(8192, np.float32)
    out = np.zeros(8192, np.float32)
    pcm = np.zeros(8192, np.int16)
    a, o, q = buf.ctypes.data, out.ctypes.data, pcm.ctypes.data
    proc = lib.kq_mon_process
    assert proc(bank, a, KQ_MON_F32, 0, 512, 512, 3, 0, None, 0, None, 0, None) == -1      # 1536 > 1024
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_mon_process: ") and b"max_samples 1024" in msg, msg
    assert proc(bank, a, 2, 0, 16, 16, 1, 0, None, 0, None, 0, None) == -1
    assert lib.kq_last_error() == b"kq_mon_process: unknown format 2"
    assert proc(bank, a, -1, 0, 16, 16, 1, 0, None, 0, None, 0, None) == -1
    assert lib.kq_last_error() == b"kq_mon_process: unknown format -1"
    assert proc(bank, a, KQ_MON_S16BE, 0, 100, 200, 2, 0, None, 0, None, 0, None) == -1
    assert b"kq_mon_process: row_stride 100 < 200" in lib.kq_last_error()
    # a stereo session reads 2 block_len elements of every block
    assert lib.kq_mon_set(bank, 1, C.byref(mon_params(channels=2))) == 0
    assert proc(bank, a, KQ_MON_F32, 0, 300, 200, 2, 0, None, 0, None, 0, None) == -1
    msg = lib.kq_last_error()
    assert b"kq_mon_process: row_stride 300 < 400" in msg and b"stereo" in msg, msg
    assert lib.kq_mon_remove(bank, 1) == 0
    assert proc(bank, a, KQ_MON_F32, 0, 64, 64, 1, 0, o, 100, None, 0, None) == -1
    assert b"kq_mon_process: out_stride 100 < 2 T = 128" in lib.kq_last_error()
    assert proc(bank, a, KQ_MON_F32, 0, 64, 64, 1, 0, None, 0, q, 127, None) == -1
    assert b"kq_mon_process: pcm_stride 127 < 2 T = 128" in lib.kq_last_error()
    assert proc(bank, None, KQ_MON_F32, 0, 16, 16, 1, 0, None, 0, None, 0, None) == -1
    assert lib.kq_last_error() == b"kq_mon_process: null audio"
    assert proc(bank, None, KQ_MON_F32, 0, 0, 0, 0, 0, None, 0, None, 0, None) == 0          # nothing to do
    assert proc(None, a, KQ_MON_F32, 0, 16, 16, 1, 0, None, 0, None, 0, None) == -1
    assert lib.kq_last_error() == b"kq_mon_process: null bank"


def test_null_handles_refused(lib):
    for fn, args in ((lib.kq_mon_destroy, ()), (lib.kq_mon_sync, ()), (lib.kq_mon_reset, ()), (lib.kq_mon_remove, (0,)),
                     (lib.kq_mon_adjust, (0, 1.0, 0.0, 0))):
        assert fn(None, *args) == -1
        assert b"null bank" in lib.kq_last_error()
