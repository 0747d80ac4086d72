"""Argument checks of the NAVTEX decoder bank (kq_navtex_*): every limit is refused with -1 / NULL and a reason that names
the function and the field before any HIP call, so they hold without a GPU (kq_navtex_create, kq_navtex_set and
kq_navtex_remove touch no device: the next call does); the cosine table, the phase increments, the bit length and the window
the bank hands out against the model's; and the record layouts against the dtypes."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import navtex_model as nm
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import ccir476
from ka9q_sdr_amd.navtex import (EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, NavtexConfig, NavtexParams, NavtexSlot, _bind,
                                 navtex_params)


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the limits of baud themselves; the getter's own refusals"""
    out = NavtexSlot()
    assert lib.kq_navtex_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    for baud, tb in ((125.0, 2048), (31.25, 8192), (100.0, 2560)):
        assert lib.kq_navtex_set(bank, 1, C.byref(navtex_params(baud=baud))) == 0, lib.kq_last_error()
        assert lib.kq_navtex_get_slot(bank, 1, C.byref(out)) == 0 and out.tb == tb and out.W == tb // 256
    assert lib.kq_navtex_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_navtex_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_navtex_get_slot: null out"
    assert lib.kq_navtex_remove(bank, 1) == 0


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "navtex", NavtexConfig, navtex_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,),
    null_pull=b"null event",
    default=dict(device=0, samprate=12000.0, block_len=12, warm=64, snr=64, min_p=1 << 16, input_scale=32767.0, max_slots=8,
                 max_events=4, max_samples=1 << 14, stream=None, acq=4, pairs=4, lose=16),
    bad_configs=[
        (dict(samprate=0.0), b"samprate 0 must be positive and finite"),
        (dict(samprate=-8000.0), b"samprate -8000"),
        (dict(samprate=float("nan")), b"samprate nan"),
        (dict(samprate=float("inf")), b"samprate inf"),
        (dict(block_len=7), b"block_len 7 must be 8..256"),
        (dict(block_len=257), b"block_len 257 must be 8..256"),
        (dict(warm=65536), b"warm 65536 must be 0..65535"),
        (dict(snr=15), b"snr 15 must be 16..4095"),
        (dict(snr=4096), b"snr 4096 must be 16..4095"),
        (dict(min_p=(1 << 55) + 1), b"min_p 36028797018963969 must be 0..2^55"),
        (dict(input_scale=0.0), b"input_scale"),
        (dict(input_scale=-1.0), b"input_scale"),
        (dict(input_scale=float("nan")), b"input_scale"),
        (dict(input_scale=float("inf")), b"input_scale"),
        (dict(acq=2), b"acq 2 must be 3..4"),
        (dict(acq=5), b"acq 5 must be 3..4"),
        (dict(pairs=2), b"pairs 2 must be 3..6"),
        (dict(pairs=7), b"pairs 7 must be 3..6"),
        (dict(lose=0), b"lose 0 must be 1..255"),
        (dict(lose=256), b"lose 256 must be 1..255"),
        (dict(max_slots=0), b"max_slots 0 must be 1..16384"),
        (dict(max_slots=16385), b"max_slots 16385"),
        (dict(max_events=0), b"max_events 0 must be 1..4096"),
        (dict(max_events=4097), b"max_events 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
    ],
    bad_params=[
        (dict(mark=0.0), b"mark 0 must be above 0 and below samprate / 2"), (dict(mark=6000.0), b"mark 6000"),
        (dict(mark=-1.0), b"mark -1"), (dict(mark=float("nan")), b"mark nan"),
        (dict(space=0.0), b"space 0 must be above 0 and below samprate / 2"), (dict(space=6000.0), b"space 6000"),
        (dict(space=float("nan")), b"space nan"), (dict(mark=1700.0, space=1700.0), b"mark and space are both 1700"),
        (dict(baud=0.0), b"baud 0 must be positive and finite"), (dict(baud=float("nan")), b"baud nan"),
        (dict(baud=float("inf")), b"baud inf"),
        # B = 12 at 12 kHz: 150 baud is 6.67 frames a bit, 30 baud 33.3; 125 and 31.25 are the limits
        (dict(baud=150.0), b"baud 150 makes tb 1707"), (dict(baud=125.2), b"outside 2048..8192"),
        (dict(baud=30.0), b"baud 30 makes tb 8533"), (dict(baud=31.2), b"outside 2048..8192")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_slot", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.NavtexBank, geometry=(12000.0, 12), set=dict(source=0, mark=1785.0, space=1615.0, baud=100.0),
                    read=lambda b: b.get_slot(0), want=(nm.navtex_inc(1785.0, 12000.0), nm.navtex_inc(1615.0, 12000.0), 2560, 10),
                    refused=[((12000.0, 512), {}, "block_len 512 must be 8..256"), ((12000.0, 12), dict(acq=2), "acq 2 must be 3..4"),
                             ((12000.0, 12), dict(pairs=7), "pairs 7 must be 3..6")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_navtex_create", "kq_navtex_destroy", "kq_navtex_set", "kq_navtex_remove", "kq_navtex_process",
         "kq_navtex_pull_counts", "kq_navtex_pull_event", "kq_navtex_clear_events", "kq_navtex_get_table", "kq_navtex_get_slot",
         "kq_navtex_sync", "kq_navtex_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_navtex_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.NavtexBank and kq.NavtexParams and kq.navtex_params and kq.ccir476.modulate and kq.ccir476.read_text
    assert kq.ccir476.messages and kq.ccir476.navtex_config and kq.navtex.status_array and kq.navtex.EVENT_DTYPE


def test_record_layouts():
    """kq_navtex_status is 192 bytes, 48 words, and goes through one lane whole; kq_navtex_event is 40 bytes"""
    assert STATUS_DTYPE.itemsize == 192 and STATUS_WORDS == 48 and EVENT_DTYPE.itemsize == 40 and EVENT_DTYPE.itemsize % 8 == 0
    f = STATUS_DTYPE.fields
    assert f["t"][1] == 8 and f["bitpos"][1] == 24 and f["kind"][1] == 28 and f["run"][1] == 36 and f["events"][1] == 40
    assert f["tsyncs"][1] == 52 and f["idles"][1] == 60 and f["sig"][1] == 64 and f["r_hi"][1] == 128 and f["r_lo"][1] == 136
    assert f["sum"][1] == 144 and f["acc"][1] == 160
    e = EVENT_DTYPE.fields
    assert e["code"][1] == 0 and e["flags"][1] == 4 and e["dx"][1] == 8 and e["rx"][1] == 12 and e["end_sample"][1] == 16
    assert e["nse"][1] == 32
    assert C.sizeof(NavtexParams) == 16 and C.sizeof(NavtexConfig) == 88 and C.sizeof(NavtexSlot) == 16
    assert NavtexConfig.samprate.offset == 8 and NavtexConfig.block_len.offset == 16 and NavtexConfig.min_p.offset == 32
    assert NavtexConfig.input_scale.offset == 40 and NavtexConfig.max_samples.offset == 56 and NavtexConfig.stream.offset == 64
    assert NavtexConfig.acq.offset == 72 and NavtexConfig.pairs.offset == 76 and NavtexConfig.lose.offset == 80
    assert NavtexParams.baud.offset == 12
    assert tuple(STATUS_DTYPE.names) == nm.STATUS and kq.navtex.Event._fields == nm.Event._fields == EVENT_DTYPE.names


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=8), dict(block_len=256, samprate=48000.0 * 8), dict(samprate=39062.5, block_len=32),
               dict(samprate=48000.0, block_len=56), dict(warm=0), dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0),
               dict(min_p=1 << 55), dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1),
               dict(max_samples=1 << 28), dict(acq=3), dict(acq=4), dict(pairs=3), dict(pairs=6), dict(lose=1), dict(lose=255)):
        h = lib.kq_navtex_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_navtex_destroy(h) == 0
    for fs in (12000.0, 39062.5, 48000.0):
        b = kq.NavtexBank(fs, max_slots=4, max_samples=4096, **ccir476.navtex_config(fs))
        b.set(0)
        assert b.get_slot(0).W == 10
        b.close()


@pytest.mark.parametrize("Fs,B", [(12000.0, 12), (12000.0, 8), (39062.5, 32), (48000.0, 56)])
def test_table_and_slot_match_the_model(lib, Fs, B):
    """C, inc_m, inc_s, tb and W are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_navtex_create(C.byref(_cfg(samprate=Fs, block_len=B)))
    assert h, lib.kq_last_error()
    tab = np.zeros(nm.TABLE + 2, np.int16)
    assert lib.kq_navtex_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()        # cap is kept
    assert lib.kq_navtex_get_table(h, tab.ctypes.data, nm.TABLE + 2) == 1024 and not tab[nm.TABLE:].any()
    assert np.array_equal(tab[:nm.TABLE], nm.cos_table())
    out = NavtexSlot()
    lo, hi = Fs / (B * 32.0), Fs / (B * 8.0)                          # the baud rates the geometry takes
    bauds = [b for b in (45.45, 50.0, 75.0, 100.0, 110.0, 150.0, 200.0, 300.0, lo * 1.001, hi * 0.999) if lo * 1.001 <= b <= hi * 0.999]
    assert len(bauds) >= 3
    for slot, baud in enumerate(bauds[:8]):
        mark, space = (1785.0, 0.001, 1234.567, Fs / 2 - 1.0)[slot % 4], (1615.0, 399.99, 3141.59 % (Fs / 2), 50.0)[slot % 4]
        assert lib.kq_navtex_set(h, slot, C.byref(navtex_params(slot, mark, space, baud))) == 0, lib.kq_last_error()
        assert lib.kq_navtex_get_slot(h, slot, C.byref(out)) == 0
        tb = nm.bit_length(Fs, B, baud)
        assert (out.inc_m, out.inc_s, out.tb, out.W) == (nm.navtex_inc(mark, Fs), nm.navtex_inc(space, Fs), tb, nm.window(tb)), baud
        assert 8 <= out.W <= 32
    assert lib.kq_navtex_remove(h, 2) == 0 and lib.kq_navtex_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_navtex_destroy(h) == 0
