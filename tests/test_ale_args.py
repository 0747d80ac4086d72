"""Argument checks of the ALE decoder bank (kq_ale_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_ale_create, kq_ale_set and kq_ale_remove touch
no device: the next call does); and the cosine table, the eight phase increments, the symbol length and the window the
bank hands out against the model's."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import ale_model as am
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import ale2g
from ka9q_sdr_amd.ale import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, AleConfig, AleParams, AleSlot, _bind, ale_params


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the limits of baud themselves, an LSB channel; the getter's
    own refusals"""
    out = AleSlot()
    assert lib.kq_ale_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    for baud, tb in ((125.0, 2048), (31.25, 8192)):
        assert lib.kq_ale_set(bank, 1, C.byref(ale_params(baud=baud))) == 0, lib.kq_last_error()
        assert lib.kq_ale_get_slot(bank, 1, C.byref(out)) == 0 and out.tb == tb and out.W == tb // 256
    assert lib.kq_ale_set(bank, 2, C.byref(ale_params(f0=2500.0, df=-250.0))) == 0, lib.kq_last_error()   # an LSB channel
    assert lib.kq_ale_get_slot(bank, 2, C.byref(out)) == 0 and list(out.inc) == list(reversed(am.ale_inc(750.0, 250.0, 12000.0)))
    assert lib.kq_ale_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_ale_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_ale_get_slot: null out"
    assert lib.kq_ale_remove(bank, 1) == 0


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "ale", AleConfig, ale_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,), null_pull=b"null event",
    default=dict(device=0, samprate=12000.0, block_len=12, warm=64, snr=80, min_p=1 << 16, input_scale=32767.0, max_slots=8,
                 max_events=4, max_samples=1 << 14, stream=None, acq_err=1, lose=2),
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
        (dict(acq_err=4), b"acq_err 4 must be 0..3"),
        (dict(lose=0), b"lose 0 must be 1..15"),
        (dict(lose=16), b"lose 16 must be 1..15"),
        (dict(max_slots=0), b"max_slots 0 must be 1..16384"),
        (dict(max_slots=16385), b"max_slots 16385"),
        (dict(max_events=0), b"max_events 0 must be 1..4096"),
        (dict(max_events=4097), b"max_events 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
    ],
    bad_params=[
        (dict(f0=0.0), b"tone 0 at 0 (f0 0, df 250) must be above 0 and below samprate / 2"), (dict(f0=-1.0), b"tone 0 at -1"),
        (dict(f0=4250.0), b"tone 7 at 6000"), (dict(f0=1750.0, df=-250.0), b"tone 7 at 0"),
        (dict(f0=6000.0, df=-250.0), b"tone 0 at 6000"),
        (dict(df=0.0), b"df 0 must be finite and df not 0"), (dict(f0=float("nan")), b"f0 nan"), (dict(df=float("inf")), b"df inf"),
        (dict(baud=0.0), b"baud 0 must be positive and finite"), (dict(baud=-125.0), b"baud -125"),
        (dict(baud=float("nan")), b"baud nan"), (dict(baud=float("inf")), b"baud inf"),
        # B = 12 at 12 kHz: 250 baud is 4 frames a symbol, 30 baud 33.3; 125 and 31.25 are the limits themselves
        (dict(baud=250.0), b"baud 250 makes tb 1024"), (dict(baud=125.2), b"outside 2048..8192"),
        (dict(baud=30.0), b"baud 30 makes tb 8533"), (dict(baud=31.2), b"outside 2048..8192")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_slot", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.AleBank, geometry=(12000.0, 12), set=dict(source=0, f0=750.0, df=250.0, baud=125.0),
                    read=lambda b: b.get_slot(0), want=(tuple(am.ale_inc(750.0, 250.0, 12000.0)), 2048, 8), again=dict(),
                    refused=[((12000.0, 512), {}, "block_len 512 must be 8..256")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_ale_create", "kq_ale_destroy", "kq_ale_set", "kq_ale_remove", "kq_ale_process", "kq_ale_pull_counts",
         "kq_ale_pull_event", "kq_ale_clear_events", "kq_ale_get_table", "kq_ale_get_slot", "kq_ale_sync", "kq_ale_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_ale_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.AleBank and kq.AleParams and kq.ale_params and kq.ale2g.word_symbols and kq.ale2g.read
    assert kq.ale2g.modulate and kq.ale2g.ale_config and kq.ale2g.individual_call and kq.ale.status_array and kq.ale.EVENT_DTYPE


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 320 and STATUS_WORDS == 80 and EVENT_DTYPE.itemsize == 48
    f = STATUS_DTYPE.fields
    assert f["t"][1] == 8 and f["nsym"][1] == 16 and f["synced"][1] == 28 and f["dropped"][1] == 40 and f["sig"][1] == 48
    assert f["nse"][1] == 56 and f["ee"][1] == 64 and f["pe"][1] == 80 and f["oth"][1] == 96 and f["r0"][1] == 104
    assert f["r2"][1] == 120 and f["sum"][1] == 128 and f["acc"][1] == 192
    e = EVENT_DTYPE.fields
    assert e["err_a"][1] == 8 and e["split"][1] == 16 and e["end_sample"][1] == 24 and e["sig"][1] == 32 and e["nse"][1] == 40
    assert C.sizeof(AleParams) == 16 and C.sizeof(AleConfig) == 80 and C.sizeof(AleSlot) == 40
    assert AleConfig.samprate.offset == 8 and AleConfig.block_len.offset == 16 and AleConfig.min_p.offset == 32
    assert AleConfig.input_scale.offset == 40 and AleConfig.max_samples.offset == 56 and AleConfig.stream.offset == 64
    assert AleConfig.acq_err.offset == 72 and AleConfig.lose.offset == 76
    assert AleParams.f0.offset == 4 and AleParams.df.offset == 8 and AleParams.baud.offset == 12 and AleSlot.tb.offset == 32
    assert tuple(STATUS_DTYPE.names) == am.STATUS and tuple(EVENT_DTYPE.names) == am.Event._fields


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=8), dict(block_len=256, samprate=512000.0), dict(samprate=39062.5, block_len=32),
               dict(samprate=96000.0, block_len=96), dict(warm=0), dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0),
               dict(min_p=1 << 55), dict(acq_err=0), dict(acq_err=3), dict(lose=1), dict(lose=15),
               dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1), dict(max_samples=1 << 28)):
        h = lib.kq_ale_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_ale_destroy(h) == 0
    for fs, B in ((8000.0, 8), (12000.0, 12), (39062.5, 39), (48000.0, 48), (96000.0, 96), (512000.0, 256)):
        assert ale2g.ale_config(fs) == dict(block_len=B)
        b = kq.AleBank(fs, max_slots=4, max_samples=4096, **ale2g.ale_config(fs))
        b.set(0)
        assert b.get_slot(0).W in (8, 16)
        b.close()


@pytest.mark.parametrize("Fs,B", [(8000.0, 8), (12000.0, 8), (12000.0, 12), (39062.5, 32), (48000.0, 24), (48000.0, 48)])
def test_table_and_slot_match_the_model(lib, Fs, B):
    """C, inc[8], tb and W are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_ale_create(C.byref(_cfg(samprate=Fs, block_len=B)))
    assert h, lib.kq_last_error()
    tab = np.zeros(am.TABLE + 2, np.int16)
    assert lib.kq_ale_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()         # cap is kept
    assert lib.kq_ale_get_table(h, tab.ctypes.data, am.TABLE + 2) == 1024 and not tab[am.TABLE:].any()
    assert np.array_equal(tab[:am.TABLE], am.cos_table())
    out = AleSlot()
    plans = [(750.0, 250.0, 125.0), (790.0, 250.0, 125.0), (2500.0, -250.0, 125.0), (0.001, 250.0, 125.0),
             (1234.567, 123.4567, 125.0 * 1.0001), (Fs / 2 - 1.0, -(Fs / 2 - 2.0) / 7.0, 125.0 * 0.999)]
    for slot, (f0, df, baud) in enumerate(plans):
        assert lib.kq_ale_set(h, slot, C.byref(ale_params(slot, f0, df, baud))) == 0, lib.kq_last_error()
        assert lib.kq_ale_get_slot(h, slot, C.byref(out)) == 0
        tb = am.symbol_length(Fs, B, baud)
        assert (list(out.inc), out.tb, out.W) == (am.ale_inc(f0, df, Fs), tb, am.window(tb)), (f0, df, baud)
        assert 8 <= out.W <= 32
    assert lib.kq_ale_get_slot(h, 0, C.byref(out)) == 0
    assert (out.tb, out.W) == {(8000.0, 8): (2048, 8), (12000.0, 8): (3072, 12), (12000.0, 12): (2048, 8), (39062.5, 32): (2500, 10),
                               (48000.0, 24): (4096, 16), (48000.0, 48): (2048, 8)}[(Fs, B)]
    assert lib.kq_ale_remove(h, 2) == 0 and lib.kq_ale_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_ale_destroy(h) == 0
