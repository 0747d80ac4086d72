"""Argument checks of the FSK / GMSK packet decoder bank (kq_fsk_*): every limit is refused with -1 / NULL and a reason that
names the function and the field before any HIP call, so they hold without a GPU (kq_fsk_create touches no device); and
the quantised low-pass the bank designs against the model's own design."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import ka9q_sdr_amd as kq
import fsk_model as fm
from ka9q_sdr_amd.fsk import INFO_DTYPE, STATUS_DTYPE, FskConfig, FskParams, _bind, fsk_params


FRAME = np.zeros(64, np.uint8)
SUITE = bank_args.Suite(
    "fsk", FskConfig, fsk_params, _bind, status=STATUS_DTYPE, record="frame", pull=(FRAME.ctypes.data, 64, None), null_pull=b"null dst",
    slot_limit=4096, set_needs_device=True,
    default=dict(device=0, samprate=48000, baud=9600, taps=21, cutoff_hz=5760.0, kaiser_beta=2.0, window_bits=16.0,
                 input_scale=4096.0, pll_shift=3, max_slots=8, max_frames=4, max_frame_bytes=64, max_samples=1 << 14, stream=None),
    bad_configs=[
        (dict(samprate=38399), b"samprate 38399 must be 4 .. 40 times baud 9600"),
        (dict(samprate=384001), b"samprate 384001 must be 4 .. 40 times baud 9600"),
        (dict(samprate=24000), b"samprate 24000"),                         # 2.5 samples per bit
        (dict(baud=0), b"baud 0"),
        (dict(samprate=-1), b"samprate -1"),
        (dict(taps=20), b"taps 20 must be odd"),
        (dict(taps=1), b"taps 1"),
        (dict(taps=129), b"taps 129"),
        (dict(window_bits=0.2), b"window_bits 0.2 gives W = 1 samples"),
        (dict(window_bits=205.0), b"gives W = 1025 samples"),
        (dict(window_bits=float("nan")), b"window_bits"),
        (dict(window_bits=-4.0), b"window_bits"),
        (dict(cutoff_hz=0.0), b"cutoff_hz 0"),
        (dict(cutoff_hz=24000.0), b"cutoff_hz 24000"),
        (dict(cutoff_hz=float("nan")), b"cutoff_hz"),
        (dict(kaiser_beta=-1.0), b"kaiser_beta"),
        (dict(kaiser_beta=float("inf")), b"kaiser_beta"),
        (dict(pll_shift=0), b"pll_shift 0"),
        (dict(pll_shift=9), b"pll_shift 9"),
        (dict(input_scale=0.0), b"input_scale"),
        (dict(input_scale=-1.0), b"input_scale"),
        (dict(input_scale=float("nan")), b"input_scale"),
        (dict(max_slots=0), b"max_slots 0"),
        (dict(max_slots=4097), b"max_slots 4097"),
        (dict(max_frames=0), b"max_frames 0"),
        (dict(max_frame_bytes=7), b"max_frame_bytes 7"),
        (dict(max_frame_bytes=1025), b"max_frame_bytes 1025"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(samprate=38400, taps=127), b"sum |hq| = 66153 > 65535"),     # long filter, four samples per bit: could overflow
    ],
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_frames", ()), ("pull_counts", (None,)),
                  ("get_taps", (None, 0)), ("pull_frame", (0, 0, None, 0, None))])
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot


NAMES = {"kq_fsk_create", "kq_fsk_destroy", "kq_fsk_set", "kq_fsk_remove", "kq_fsk_process", "kq_fsk_pull_counts",
         "kq_fsk_pull_frame", "kq_fsk_clear_frames", "kq_fsk_get_taps", "kq_fsk_sync", "kq_fsk_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_fsk_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.FskBank and kq.fsk_params and kq.ais_nmea


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 32 and INFO_DTYPE.itemsize == 16
    assert STATUS_DTYPE.fields["pll_phase"][1] == 20 and STATUS_DTYPE.fields["level"][1] == 28
    assert INFO_DTYPE.fields["end_bit"][1] == 4 and INFO_DTYPE.fields["end_sample"][1] == 8
    assert C.sizeof(FskParams) == 12 and C.sizeof(FskConfig) == 64
    assert FskConfig.max_samples.offset == 48 and FskConfig.stream.offset == 56


def test_good_configs_accepted(lib):
    for kw in (dict(), dict(samprate=38400), dict(samprate=384000, window_bits=25.6),   # Fs = 4 and 40 baud; W = 1024
               dict(samprate=39062, taps=17), dict(taps=3), dict(taps=127), dict(window_bits=0.4),     # W = 2
               dict(baud=1200, taps=127, cutoff_hz=720.0), dict(pll_shift=1), dict(pll_shift=8),
               dict(max_slots=4096, max_frames=1, max_frame_bytes=8), dict(max_frame_bytes=1024), dict(cutoff_hz=23999.0)):
        h = lib.kq_fsk_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_fsk_destroy(h) == 0


def test_bad_params_refused(lib, bank):
    for mb in (0, 3):
        p = fsk_params(min_bytes=mb)
        for h in (None, bank):   # checked before the bank is looked at
            assert lib.kq_fsk_set(h, 0, C.byref(p)) == -1
            msg = lib.kq_last_error()
            assert msg.startswith(b"kq_fsk_set: ") and b"min_bytes %d" % mb in msg, msg
    assert lib.kq_fsk_set(bank, 0, C.byref(fsk_params(min_bytes=65))) == -1      # max_frame_bytes = 64
    assert lib.kq_last_error() == b"kq_fsk_set: min_bytes 65 > max_frame_bytes 64"


@pytest.mark.parametrize("kw", [dict(), dict(samprate=39062, taps=17), dict(samprate=96000, taps=41, kaiser_beta=3.5),
                                dict(baud=4800, taps=41, cutoff_hz=2880.0), dict(baud=1200, taps=127, cutoff_hz=720.0),
                                dict(taps=3), dict(taps=127, kaiser_beta=6.0), dict(samprate=384000, taps=127, window_bits=25.6)])
def test_taps_match_the_models_design(lib, kw):
    """hq within one LSB of the float64 design of tests/fsk_model.py (i0 and sinc may differ in the last place, and a
    value that close to a half rounds the other way); the GPU tests hand the bank's taps to the model"""
    c = _cfg(**kw)
    h = lib.kq_fsk_create(C.byref(c))
    assert h, lib.kq_last_error()
    hq = np.zeros(c.taps + 2, np.int16)
    assert lib.kq_fsk_get_taps(h, hq.ctypes.data, 2) == c.taps and not hq[2:].any()      # cap is kept
    assert lib.kq_fsk_get_taps(h, hq.ctypes.data, c.taps + 2) == c.taps and not hq[c.taps:].any()
    assert lib.kq_fsk_destroy(h) == 0
    want = fm.design_taps(c.taps, c.cutoff_hz, c.samprate, c.kaiser_beta)
    got = hq[:c.taps].astype(np.int64)
    assert np.abs(got - want).max() <= 1 and np.array_equal(got, got[::-1]) and np.abs(got).sum() <= 65535
