"""Argument checks of the RTTY decoder bank (kq_rtty_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_rtty_create, kq_rtty_set and kq_rtty_remove
touch no device: the next call does); and the cosine table, the phase increments, the bit length and the window the bank
hands out against the model's."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import rtty_model as rm
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import baudot
from ka9q_sdr_amd.rtty import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, RttyConfig, RttyParams, RttySlot, _bind, rtty_params


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the limits of baud themselves; the getter's own refusals"""
    out = RttySlot()
    assert lib.kq_rtty_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    for baud, tb in ((62.5, 2048), (15.625, 8192)):
        assert lib.kq_rtty_set(bank, 1, C.byref(rtty_params(baud=baud))) == 0, lib.kq_last_error()
        assert lib.kq_rtty_get_slot(bank, 1, C.byref(out)) == 0 and out.tb == tb and out.W == tb // 256
    assert lib.kq_rtty_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_rtty_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_rtty_get_slot: null out"
    assert lib.kq_rtty_remove(bank, 1) == 0


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "rtty", RttyConfig, rtty_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,), null_pull=b"null event",
    default=dict(device=0, samprate=12000.0, block_len=24, warm=64, snr=96, min_p=1 << 16, input_scale=32767.0, max_slots=8,
                 max_events=4, max_samples=1 << 14, stream=None),
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
        (dict(space=float("nan")), b"space nan"), (dict(mark=2125.0, space=2125.0), b"mark and space are both 2125"),
        (dict(nbits=4), b"nbits 4 must be 5..8"), (dict(nbits=9), b"nbits 9 must be 5..8"),
        (dict(baud=0.0), b"baud 0 must be positive and finite"), (dict(baud=float("nan")), b"baud nan"),
        (dict(baud=float("inf")), b"baud inf"),
        # B = 24 at 12 kHz: 75 baud is 6.67 frames a bit, 15 baud 33.3; 62.5 and 15.625 are the limits themselves
        (dict(baud=75.0), b"baud 75 makes tb 1707"), (dict(baud=62.6), b"outside 2048..8192"),
        (dict(baud=15.0), b"baud 15 makes tb 8533"), (dict(baud=15.6), b"outside 2048..8192")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_slot", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.RttyBank, geometry=(12000.0, 24), set=dict(source=0, mark=2125.0, space=2295.0, baud=45.45),
                    read=lambda b: b.get_slot(0), want=(rm.rtty_inc(2125.0, 12000.0), rm.rtty_inc(2295.0, 12000.0), 2816, 11),
                    refused=[((12000.0, 512), {}, "block_len 512 must be 8..256")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_rtty_create", "kq_rtty_destroy", "kq_rtty_set", "kq_rtty_remove", "kq_rtty_process", "kq_rtty_pull_counts",
         "kq_rtty_pull_event", "kq_rtty_clear_events", "kq_rtty_get_table", "kq_rtty_get_slot", "kq_rtty_sync", "kq_rtty_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_rtty_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.RttyBank and kq.RttyParams and kq.rtty_params and kq.baudot.encode and kq.baudot.read_text
    assert kq.baudot.codes_of and kq.baudot.rtty_config and kq.rtty.status_array and kq.rtty.EVENT_DTYPE


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 112 and STATUS_WORDS == 28 and EVENT_DTYPE.itemsize == 32
    f = STATUS_DTYPE.fields
    assert f["bit"][1] == 8 and f["t"][1] == 16 and f["false_starts"][1] == 32 and f["sig"][1] == 40 and f["start"][1] == 56
    assert f["sum_im"][1] == 64 and f["sum_qs"][1] == 76 and f["acc_im"][1] == 80 and f["acc_qs"][1] == 104
    assert EVENT_DTYPE.fields["start_sample"][1] == 8 and EVENT_DTYPE.fields["sig"][1] == 16 and EVENT_DTYPE.fields["nse"][1] == 24
    assert C.sizeof(RttyParams) == 20 and C.sizeof(RttyConfig) == 72 and C.sizeof(RttySlot) == 16
    assert RttyConfig.samprate.offset == 8 and RttyConfig.block_len.offset == 16 and RttyConfig.min_p.offset == 32
    assert RttyConfig.input_scale.offset == 40 and RttyConfig.max_samples.offset == 56 and RttyConfig.stream.offset == 64
    assert RttyParams.baud.offset == 12 and RttyParams.nbits.offset == 16
    assert tuple(STATUS_DTYPE.names) == rm.STATUS


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=8), dict(block_len=256, samprate=48000.0 * 8), dict(samprate=39062.5, block_len=64),
               dict(samprate=48000.0, block_len=128), dict(warm=0), dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0),
               dict(min_p=1 << 55), dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1),
               dict(max_samples=1 << 28)):
        h = lib.kq_rtty_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_rtty_destroy(h) == 0
    for fs, baud in ((12000.0, 45.45), (12000.0, 75.0), (39062.5, 50.0), (48000.0, 100.0)):
        b = kq.RttyBank(fs, max_slots=4, max_samples=4096, **baudot.rtty_config(fs, baud))
        b.set(0, baud=baud)
        assert b.get_slot(0).W in (10, 11)
        b.close()


@pytest.mark.parametrize("Fs,B", [(12000.0, 24), (39062.5, 64), (48000.0, 128), (12000.0, 8), (8000.0, 16)])
def test_table_and_slot_match_the_model(lib, Fs, B):
    """C, inc_m, inc_s, tb and W are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_rtty_create(C.byref(_cfg(samprate=Fs, block_len=B)))
    assert h, lib.kq_last_error()
    tab = np.zeros(rm.TABLE + 2, np.int16)
    assert lib.kq_rtty_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()        # cap is kept
    assert lib.kq_rtty_get_table(h, tab.ctypes.data, rm.TABLE + 2) == 1024 and not tab[rm.TABLE:].any()
    assert np.array_equal(tab[:rm.TABLE], rm.cos_table())
    out = RttySlot()
    lo, hi = Fs / (B * 32.0), Fs / (B * 8.0)                          # the baud rates the geometry takes
    bauds = [b for b in (45.45, 50.0, 56.92, 75.0, 100.0, 110.0, 150.0, 200.0, 300.0, lo * 1.001, hi * 0.999) if lo * 1.001 <= b <= hi * 0.999]
    assert len(bauds) >= 3
    for slot, baud in enumerate(bauds[:8]):
        mark, space = (2125.0, 0.001, 1234.567, Fs / 2 - 1.0)[slot % 4], (2295.0, 399.99, 3141.59 % (Fs / 2), 50.0)[slot % 4]
        assert lib.kq_rtty_set(h, slot, C.byref(rtty_params(slot, mark, space, baud, 5 + slot % 4))) == 0, lib.kq_last_error()
        assert lib.kq_rtty_get_slot(h, slot, C.byref(out)) == 0
        tb = rm.bit_length(Fs, B, baud)
        assert (out.inc_m, out.inc_s, out.tb, out.W) == (rm.rtty_inc(mark, Fs), rm.rtty_inc(space, Fs), tb, rm.window(tb)), baud
        assert abs(out.inc_m * Fs / 2.0 ** 32 - float(np.float32(mark))) < Fs / 2.0 ** 32 and 8 <= out.W <= 32
    assert lib.kq_rtty_remove(h, 2) == 0 and lib.kq_rtty_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_rtty_destroy(h) == 0
