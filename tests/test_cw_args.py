"""Argument checks of the CW decoder bank (kq_cw_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_cw_create, kq_cw_set and kq_cw_remove touch no
device: the next call does); and the cosine table and the phase increments the bank hands out against the model's."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import cw_model as cm
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import morse
from ka9q_sdr_amd.cw import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, CwConfig, CwParams, _bind, cw_params


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the getter's own refusals"""
    inc = np.zeros(1, np.uint32)
    assert lib.kq_cw_get_inc(bank, 0, inc.ctypes.data) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    assert lib.kq_cw_get_inc(bank, 8, inc.ctypes.data) == -1 and lib.kq_cw_get_inc(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_cw_get_inc: null inc"


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "cw", CwConfig, cw_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,), null_pull=b"null event",
    default=dict(device=0, samprate=12000.0, block_len=48, min_wpm=5.0, max_wpm=60.0, deb=2, warm=64, snr=256, min_p=1 << 16,
                 input_scale=32767.0, max_slots=8, max_events=4, max_samples=1 << 14, stream=None),
    bad_configs=[
        (dict(samprate=0.0), b"samprate 0 must be positive and finite"),
        (dict(samprate=-8000.0), b"samprate -8000"),
        (dict(samprate=float("nan")), b"samprate nan"),
        (dict(samprate=float("inf")), b"samprate inf"),
        (dict(block_len=7), b"block_len 7 must be 8..4096"),
        (dict(block_len=4097), b"block_len 4097 must be 8..4096"),
        (dict(min_wpm=0.0), b"speeds 0..60 WPM must be positive, finite and in order"),
        (dict(min_wpm=-5.0), b"speeds -5..60 WPM"),
        (dict(min_wpm=30.0, max_wpm=20.0), b"speeds 30..20 WPM"),
        (dict(max_wpm=float("inf")), b"speeds 5..inf WPM"),
        (dict(max_wpm=float("nan")), b"speeds 5..nan WPM"),
        (dict(min_wpm=float("nan")), b"speeds nan..60 WPM"),
        (dict(max_wpm=101.0), b"max_wpm 101 leaves a dot 47 sixteenths of a frame of 48 samples, fewer than 48"),
        (dict(block_len=4096, max_wpm=20.0), b"fewer than 48"),
        (dict(block_len=8, min_wpm=0.01, samprate=48000.0), b"min_wpm 0.01 makes a dot"),
        (dict(deb=0), b"deb 0 must be 1..16"),
        (dict(deb=17), b"deb 17 must be 1..16"),
        (dict(warm=65536), b"warm 65536 must be 0..65535"),
        (dict(snr=15), b"snr 15 must be 16..4095"),
        (dict(snr=4096), b"snr 4096 must be 16..4095"),
        (dict(min_p=(1 << 55) + 1), b"min_p 36028797018963969 must be 0..2^55"),
        (dict(input_scale=0.0), b"input_scale"),
        (dict(input_scale=-1.0), b"input_scale"),
        (dict(input_scale=float("nan")), b"input_scale"),
        (dict(input_scale=float("inf")), b"input_scale"),
        (dict(max_slots=0), b"max_slots 0 must be 1..16384"),
        (dict(max_slots=16385), b"max_slots 16385"),
        (dict(max_events=0), b"max_events 0 must be 1..4096"),
        (dict(max_events=4097), b"max_events 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
    ],
    bad_params=[
        (dict(pitch=0.0), b"pitch 0 must be above 0 and below samprate / 2"), (dict(pitch=6000.0), b"pitch 6000"),
        (dict(pitch=-700.0), b"pitch -700"), (dict(pitch=float("nan")), b"pitch nan"),
        (dict(wpm=4.0), b"wpm 4 must be within the bank's 5..60"), (dict(wpm=61.0), b"wpm 61"), (dict(wpm=float("nan")), b"wpm nan")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_inc", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.CwBank, geometry=(12000.0, 48), set=dict(source=0, pitch=700.0, wpm=20.0),
                    read=lambda b: b.get_inc(0), want=cm.cw_inc(700.0, 12000.0), refused=[((12000.0, 480), {}, "fewer than 48")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_cw_create", "kq_cw_destroy", "kq_cw_set", "kq_cw_remove", "kq_cw_process", "kq_cw_pull_counts",
         "kq_cw_pull_event", "kq_cw_clear_events", "kq_cw_get_table", "kq_cw_get_inc", "kq_cw_sync", "kq_cw_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_cw_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.CwBank and kq.CwParams and kq.cw_params and kq.morse.encode and kq.morse.read_text and kq.morse.cw_config


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 88 and STATUS_WORDS == 22 and EVENT_DTYPE.itemsize == 40
    assert STATUS_DTYPE.fields["flags"][1] == 36 and STATUS_DTYPE.fields["hi"][1] == 40 and STATUS_DTYPE.fields["acc_q"][1] == 80
    assert EVENT_DTYPE.fields["start_sample"][1] == 16 and EVENT_DTYPE.fields["peak"][1] == 32
    assert C.sizeof(CwParams) == 12 and C.sizeof(CwConfig) == 80
    assert CwConfig.samprate.offset == 8 and CwConfig.min_wpm.offset == 20 and CwConfig.min_p.offset == 40
    assert CwConfig.input_scale.offset == 48 and CwConfig.max_samples.offset == 64 and CwConfig.stream.offset == 72


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=8), dict(block_len=4096, samprate=48000.0 * 64, max_wpm=60.0),
               dict(samprate=39062.5, block_len=128), dict(block_len=1024, samprate=48000.0, max_wpm=15.0),
               dict(max_wpm=80.0), dict(min_wpm=60.0), dict(min_wpm=0.05, block_len=8), dict(deb=1), dict(deb=16), dict(warm=0),
               dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0), dict(min_p=1 << 55),
               dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1), dict(max_samples=1 << 28)):
        h = lib.kq_cw_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_cw_destroy(h) == 0
    for fs, top in ((12000.0, 75.0), (12000.0, 60.0), (39062.5, 60.0), (48000.0, 40.0)):
        try:
            kq.CwBank(fs, max_slots=4, max_samples=4096, **morse.cw_config(fs, top)).close()
        except kq.KqError as e:
            raise AssertionError("%g Hz, %g WPM: %s" % (fs, top, e))


@pytest.mark.parametrize("Fs", [12000.0, 39062.5, 48000.0, 8000.0])
def test_table_and_inc_match_the_model(lib, Fs):
    """C and inc are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_cw_create(C.byref(_cfg(samprate=Fs, block_len=32)))
    assert h, lib.kq_last_error()
    tab = np.zeros(cm.TABLE + 2, np.int16)
    assert lib.kq_cw_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()        # cap is kept
    assert lib.kq_cw_get_table(h, tab.ctypes.data, cm.TABLE + 2) == 1024 and not tab[cm.TABLE:].any()
    assert np.array_equal(tab[:cm.TABLE], cm.cos_table())
    inc = np.zeros(1, np.uint32)
    for slot, pitch in enumerate((700.0, 399.99, 0.001, 1234.567, 600.1, Fs / 2 - 1.0, 3141.59, 50.0)):
        assert lib.kq_cw_set(h, slot, C.byref(cw_params(source=slot, pitch=pitch))) == 0, lib.kq_last_error()
        assert lib.kq_cw_get_inc(h, slot, inc.ctypes.data) == 0
        assert int(inc[0]) == cm.cw_inc(pitch, Fs), pitch
        assert abs(int(inc[0]) * Fs / 2.0 ** 32 - float(np.float32(pitch))) < Fs / 2.0 ** 32
    assert lib.kq_cw_remove(h, 2) == 0 and lib.kq_cw_get_inc(h, 2, inc.ctypes.data) == -1
    assert lib.kq_cw_destroy(h) == 0
