"""Argument checks of the PSK decoder bank (kq_psk_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_psk_create, kq_psk_set and kq_psk_remove touch
no device: the next call does); and the cosine table, the phase increment, the symbol length and the window the bank
hands out against the model's."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import psk_model as pm
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import varicode
from ka9q_sdr_amd.psk import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, PskConfig, PskParams, PskSlot, _bind, psk_params


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the limits of baud themselves; the getter's own refusals"""
    out = PskSlot()
    assert lib.kq_psk_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    for baud, tb in ((62.5, 2048), (15.625, 8192)):
        assert lib.kq_psk_set(bank, 1, C.byref(psk_params(baud=baud))) == 0, lib.kq_last_error()
        assert lib.kq_psk_get_slot(bank, 1, C.byref(out)) == 0 and out.tb == tb and out.W == tb // 256 and out.reserved == 0
    assert lib.kq_psk_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_psk_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_psk_get_slot: null out"
    assert lib.kq_psk_remove(bank, 1) == 0


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "psk", PskConfig, psk_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,), null_pull=b"null event",
    default=dict(device=0, samprate=12000.0, block_len=24, warm=64, snr=32, min_p=1 << 16, input_scale=32767.0, max_slots=8,
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
        (dict(pitch=0.0), b"pitch 0 must be above 0 and below samprate / 2"), (dict(pitch=6000.0), b"pitch 6000"),
        (dict(pitch=-1.0), b"pitch -1"), (dict(pitch=float("nan")), b"pitch nan"), (dict(pitch=float("inf")), b"pitch inf"),
        (dict(baud=0.0), b"baud 0 must be positive and finite"), (dict(baud=-31.25), b"baud -31.25"),
        (dict(baud=float("nan")), b"baud nan"), (dict(baud=float("inf")), b"baud inf"),
        # B = 24 at 12 kHz: 125 baud is 4 frames a symbol, 15 baud 33.3; 62.5 and 15.625 are the limits themselves
        (dict(baud=125.0), b"baud 125 makes tb 1024"), (dict(baud=62.6), b"outside 2048..8192"),
        (dict(baud=15.0), b"baud 15 makes tb 8533"), (dict(baud=15.6), b"outside 2048..8192")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_slot", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.PskBank, geometry=(12000.0, 24), set=dict(source=0, pitch=1500.0, baud=31.25),
                    read=lambda b: b.get_slot(0), want=(pm.psk_inc(1500.0, 12000.0), 4096, 16),
                    again=dict(source=0, pitch=1500.0, baud=31.25), refused=[((12000.0, 512), {}, "block_len 512 must be 8..256")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_psk_create", "kq_psk_destroy", "kq_psk_set", "kq_psk_remove", "kq_psk_process", "kq_psk_pull_counts",
         "kq_psk_pull_event", "kq_psk_clear_events", "kq_psk_get_table", "kq_psk_get_slot", "kq_psk_sync", "kq_psk_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_psk_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.PskBank and kq.PskParams and kq.psk_params and kq.varicode.encode and kq.varicode.read_text
    assert kq.varicode.modulate and kq.varicode.psk_config and kq.varicode.offset_hz and kq.psk.status_array and kq.psk.EVENT_DTYPE


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 144 and STATUS_WORDS == 36 and EVENT_DTYPE.itemsize == 32
    f = STATUS_DTYPE.fields
    assert f["t"][1] == 8 and f["dropped"][1] == 24 and f["sig"][1] == 32 and f["qim"][1] == 48 and f["ee"][1] == 56
    assert f["pe"][1] == 72 and f["pc"][1] == 80 and f["rot_r"][1] == 88 and f["cr"][1] == 104 and f["pi"][1] == 116
    assert f["sum_i"][1] == 120 and f["sum_q"][1] == 124 and f["acc_i"][1] == 128 and f["acc_q"][1] == 136
    assert EVENT_DTYPE.fields["end_sample"][1] == 8 and EVENT_DTYPE.fields["sig"][1] == 16
    assert EVENT_DTYPE.fields["rot_r"][1] == 24 and EVENT_DTYPE.fields["rot_i"][1] == 28
    assert C.sizeof(PskParams) == 12 and C.sizeof(PskConfig) == 72 and C.sizeof(PskSlot) == 16
    assert PskConfig.samprate.offset == 8 and PskConfig.block_len.offset == 16 and PskConfig.min_p.offset == 32
    assert PskConfig.input_scale.offset == 40 and PskConfig.max_samples.offset == 56 and PskConfig.stream.offset == 64
    assert PskParams.pitch.offset == 4 and PskParams.baud.offset == 8
    assert tuple(STATUS_DTYPE.names) == pm.STATUS


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=8), dict(block_len=256, samprate=48000.0), dict(samprate=39062.5, block_len=50),
               dict(samprate=48000.0, block_len=192), dict(warm=0), dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0),
               dict(min_p=1 << 55), dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1),
               dict(max_samples=1 << 28)):
        h = lib.kq_psk_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_psk_destroy(h) == 0
    for fs, baud in ((12000.0, 31.25), (12000.0, 62.5), (12000.0, 125.0), (8000.0, 31.25), (39062.5, 31.25), (48000.0, 31.25)):
        b = kq.PskBank(fs, max_slots=4, max_samples=4096, **varicode.psk_config(fs, baud))
        b.set(0, baud=baud)
        assert b.get_slot(0).W in (12, 16)
        b.close()


@pytest.mark.parametrize("Fs,B", [(12000.0, 24), (39062.5, 50), (48000.0, 192), (12000.0, 8), (8000.0, 16), (48000.0, 256)])
def test_table_and_slot_match_the_model(lib, Fs, B):
    """C, inc, tb and W are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_psk_create(C.byref(_cfg(samprate=Fs, block_len=B)))
    assert h, lib.kq_last_error()
    tab = np.zeros(pm.TABLE + 2, np.int16)
    assert lib.kq_psk_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()         # cap is kept
    assert lib.kq_psk_get_table(h, tab.ctypes.data, pm.TABLE + 2) == 1024 and not tab[pm.TABLE:].any()
    assert np.array_equal(tab[:pm.TABLE], pm.cos_table())
    out = PskSlot()
    lo, hi = Fs / (B * 32.0), Fs / (B * 8.0)                          # the baud rates the geometry takes
    bauds = [b for b in (10.0, 15.625, 31.25, 45.45, 62.5, 100.0, 125.0, 187.5, lo * 1.001, hi * 0.999) if lo * 1.001 <= b <= hi * 0.999]
    assert len(bauds) >= 3
    for slot, baud in enumerate(bauds[:8]):
        pitch = (1000.0, 0.001, 1234.567, Fs / 2 - 1.0)[slot % 4]
        assert lib.kq_psk_set(h, slot, C.byref(psk_params(slot, pitch, baud))) == 0, lib.kq_last_error()
        assert lib.kq_psk_get_slot(h, slot, C.byref(out)) == 0
        tb = pm.symbol_length(Fs, B, baud)
        assert (out.inc, out.tb, out.W) == (pm.psk_inc(pitch, Fs), tb, pm.window(tb)), baud
        assert abs(out.inc * Fs / 2.0 ** 32 - float(np.float32(pitch))) < Fs / 2.0 ** 32 and 8 <= out.W <= 32
    assert lib.kq_psk_remove(h, 2) == 0 and lib.kq_psk_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_psk_destroy(h) == 0
