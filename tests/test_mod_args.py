"""Argument checks of the modulator bank (kq_mod_*): refused with -1 / NULL and a reason before any HIP call, so they
hold without a GPU."""
import ctypes as C

import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.modulate import KQ_PCM_S16, ModConfig, _bind, station_config


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _create(lib, **kw):
    c = dict(device=0, samprate=192000, L=4096, M=4097, interp=4, max_stations=8, max_blocks=4, stream=None)
    c.update(kw)
    return lib.kq_mod_create(C.byref(ModConfig(*c.values())))


@pytest.mark.parametrize("kw,why", [
    (dict(L=4096, M=4096), b"even"),                   # N = 8191 odd
    (dict(L=4100, M=4089), b"2^a 3^b 5^c 7^d"),        # N = 8188 = 4 x 23 x 89
    (dict(L=16384, M=16385), b"16384"),                # N = 32768: past the limit
    (dict(interp=3), b"divide L"),                     # 3 does not divide L = 4096
    (dict(L=6144, M=2049, interp=3), b"M - 1"),        # N = 8192; 3 divides L = 6144 but not M - 1 = 2048
    (dict(interp=0), b"interp"),
    (dict(samprate=0), b"samprate"),
    (dict(max_stations=0), b"max_stations"),
    (dict(max_stations=70000), b"max_stations"),
    (dict(max_blocks=0), b"max_blocks"),
])
def test_bad_config_refused(lib, kw, why):
    assert _create(lib, **kw) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_mod_create") and why in msg, msg


def test_bad_slot_refused(lib):
    cfg = station_config()
    assert lib.kq_mod_set_station(None, 70000, C.byref(cfg)) == -1
    assert b"slot 70000" in lib.kq_last_error()
    assert lib.kq_mod_remove_station(None, 0) == -1


def test_bad_station_config_refused(lib):
    for bad in (dict(mod_type=7), dict(low=float("nan")), dict(low=100.0, high=-100.0), dict(frequency=float("inf"))):
        c = station_config()
        for k, v in bad.items():
            setattr(c, k, v)
        assert lib.kq_mod_set_station(None, 0, C.byref(c)) == -1
        assert lib.kq_last_error().startswith(b"kq_mod_set_station")
    assert lib.kq_mod_set_station(None, 0, None) == -1


def test_bad_format_refused(lib):
    for fmt in (1, 3, -1):   # KQ_PCM_S16BE is the AFSK decoder's wire format, not a modulator input
        assert lib.kq_mod_process(None, None, fmt, 0, 1, 0, None, None) == -1
        assert b"pcm_format" in lib.kq_last_error()
    assert lib.kq_mod_process(None, None, KQ_PCM_S16, 0, 1, 0, None, None) == -1
    assert b"null bank" in lib.kq_last_error()
