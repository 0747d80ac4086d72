"""Argument checks of the SAME decoder bank (kq_same_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_same_create, kq_same_set and kq_same_remove touch
no device: the next call does); the order in which create reports what it refuses; the cosine table, the phase increments,
the bit length and the window the bank hands out against the model's; and the record layouts against the dtypes."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import same_model as sm
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import eas
from ka9q_sdr_amd.same import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, SameConfig, SameParams, SameSlot, _bind, same_params


def _slot_checks(lib, bank):
    """behind the refused params: none of them set the slot; the limits of baud themselves; the getter's own refusals"""
    out = SameSlot()
    assert lib.kq_same_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    for baud, tb in ((750.0, 2048), (187.5, 8192), (600.0, 2560)):             # B = 8 at 48 kHz: 6000 frames a second
        assert lib.kq_same_set(bank, 1, C.byref(same_params(baud=baud))) == 0, lib.kq_last_error()
        assert lib.kq_same_get_slot(bank, 1, C.byref(out)) == 0 and out.tb == tb and out.W == tb // 256
    assert lib.kq_same_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_same_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_same_get_slot: null out"
    assert lib.kq_same_remove(bank, 1) == 0


EVENT = np.zeros(1, EVENT_DTYPE)
SUITE = bank_args.Suite(
    "same", SameConfig, same_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,),
    null_pull=b"null event",
    default=dict(device=0, samprate=48000.0, block_len=8, warm=64, snr=64, min_p=1 << 16, input_scale=32767.0, max_slots=8,
                 max_events=4, max_samples=1 << 14, stream=None, sync_errs=2, lose=3, max_len=248),
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
        (dict(sync_errs=5), b"sync_errs 5 must be 0..4"),
        (dict(sync_errs=0xFFFFFFFF), b"sync_errs 4294967295 must be 0..4"),
        (dict(lose=0), b"lose 0 must be 1..15"),
        (dict(lose=16), b"lose 16 must be 1..15"),
        (dict(max_len=7), b"max_len 7 must be 8..248"),
        (dict(max_len=249), b"max_len 249 must be 8..248"),
        (dict(max_slots=0), b"max_slots 0 must be 1..16384"),
        (dict(max_slots=16385), b"max_slots 16385"),
        (dict(max_events=0), b"max_events 0 must be 1..4096"),
        (dict(max_events=4097), b"max_events 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
        # the order: the head, then sync_errs, lose and max_len as they are declared, then the tail
        (dict(input_scale=0.0, sync_errs=5), b"input_scale"),
        (dict(sync_errs=5, lose=0, max_len=7, max_slots=0), b"sync_errs 5"),
        (dict(lose=0, max_len=7, max_slots=0), b"lose 0"),
        (dict(max_len=7, max_slots=0), b"max_len 7"),
        (dict(block_len=7, max_len=7), b"block_len 7"),
    ],
    bad_params=[
        (dict(mark=0.0), b"mark 0 must be above 0 and below samprate / 2"), (dict(mark=24000.0), b"mark 24000"),
        (dict(mark=-1.0), b"mark -1"), (dict(mark=float("nan")), b"mark nan"),
        (dict(space=0.0), b"space 0 must be above 0 and below samprate / 2"), (dict(space=24000.0), b"space 24000"),
        (dict(space=float("nan")), b"space nan"), (dict(mark=1700.0, space=1700.0), b"mark and space are both 1700"),
        (dict(baud=0.0), b"baud 0 must be positive and finite"), (dict(baud=float("nan")), b"baud nan"),
        (dict(baud=float("inf")), b"baud inf"),
        # B = 8 at 48 kHz: 800 baud is 7.5 frames a bit, 180 baud 33.3; 750 and 187.5 are the limits
        (dict(baud=800.0), b"baud 800 makes tb 1920"), (dict(baud=751.0), b"outside 2048..8192"),
        (dict(baud=180.0), b"baud 180 makes tb 8533"), (dict(baud=187.0), b"outside 2048..8192")],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_slot", (0, None)), ("pull_event", (0, 0, None))],
    first_call=dict(bank=kq.SameBank, geometry=(48000.0, 8), set=dict(source=0),
                    read=lambda b: b.get_slot(0), want=(sm.same_inc(sm.MARK, 48000.0), sm.same_inc(sm.SPACE, 48000.0), 2949, 12),
                    refused=[((48000.0, 512), {}, "block_len 512 must be 8..256"), ((48000.0, 8), dict(sync_errs=5), "sync_errs 5 must be 0..4"),
                             ((48000.0, 8), dict(max_len=249), "max_len 249 must be 8..248")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_same_create", "kq_same_destroy", "kq_same_set", "kq_same_remove", "kq_same_process", "kq_same_pull_counts",
         "kq_same_pull_event", "kq_same_clear_events", "kq_same_get_table", "kq_same_get_slot", "kq_same_sync", "kq_same_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_same_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.SameBank and kq.SameParams and kq.same_params and kq.eas.modulate and kq.eas.read and kq.eas.vote and kq.eas.parse
    assert kq.eas.header and kq.eas.burst and kq.eas.same_config and kq.same.status_array and kq.same.EVENT_DTYPE


def test_record_layouts():
    """kq_same_status is 200 bytes, 50 words of which one pads, and goes through one lane; kq_same_event is 40 bytes"""
    assert STATUS_DTYPE.itemsize == 200 and STATUS_WORDS == 50 and EVENT_DTYPE.itemsize == 40 and EVENT_DTYPE.itemsize % 8 == 0
    f = STATUS_DTYPE.fields
    assert f["t"][1] == 8 and f["bit"][1] == 12 and f["synced"][1] == 16 and f["nbytes"][1] == 24 and f["dashes"][1] == 36
    assert f["events"][1] == 40 and f["syncs"][1] == 48 and f["truncated"][1] == 64 and f["sync_sample"][1] == 72
    assert f["sig"][1] == 80 and f["lo"][1] == 136 and f["r"][1] == 144 and f["sum"][1] == 152 and f["acc"][1] == 168
    e = EVENT_DTYPE.fields
    assert e["code"][1] == 0 and e["flags"][1] == 4 and e["index"][1] == 8 and e["errs"][1] == 12 and e["end_sample"][1] == 16
    assert e["nse"][1] == 32
    assert C.sizeof(SameParams) == 16 and C.sizeof(SameConfig) == 88 and C.sizeof(SameSlot) == 16
    assert SameConfig.samprate.offset == 8 and SameConfig.block_len.offset == 16 and SameConfig.min_p.offset == 32
    assert SameConfig.input_scale.offset == 40 and SameConfig.max_samples.offset == 56 and SameConfig.stream.offset == 64
    assert SameConfig.sync_errs.offset == 72 and SameConfig.lose.offset == 76 and SameConfig.max_len.offset == 80
    assert SameParams.baud.offset == 12
    assert tuple(STATUS_DTYPE.names) == sm.STATUS and kq.same.Event._fields == sm.Event._fields == EVENT_DTYPE.names


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(block_len=11), dict(block_len=256, samprate=48000.0 * 32), dict(samprate=39062.5, block_len=9),
               dict(samprate=96000.0, block_len=23), dict(warm=0), dict(warm=65535), dict(snr=16), dict(snr=4095), dict(min_p=0),
               dict(min_p=1 << 55), dict(max_slots=16384, max_events=1), dict(max_events=4096), dict(max_samples=1),
               dict(max_samples=1 << 28), dict(sync_errs=0), dict(sync_errs=4), dict(lose=1), dict(lose=15), dict(max_len=8),
               dict(max_len=248)):
        h = lib.kq_same_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_same_destroy(h) == 0
    for fs, W in ((39062.5, 9), (48000.0, 10), (96000.0, 10)):
        b = kq.SameBank(fs, max_slots=4, max_samples=4096, **eas.same_config(fs))
        b.set(0)
        assert b.get_slot(0).W == W
        b.close()


@pytest.mark.parametrize("Fs,lo,hi", [(48000.0, 8, 11), (39062.5, 8, 9), (96000.0, 8, 23)])
def test_the_frames_a_rate_takes(lib, Fs, lo, hi):
    """the header's table: B = 8..11 at 48 kHz, 8..9 at 39 062.5 Hz, 8..23 at 96 kHz, and nothing at 24 or 12 kHz"""
    out = SameSlot()
    for B in range(8, hi + 3):
        h = lib.kq_same_create(C.byref(_cfg(samprate=Fs, block_len=B)))
        got = lib.kq_same_set(h, 0, C.byref(same_params()))
        assert got == (0 if lo <= B <= hi else -1), (Fs, B, lib.kq_last_error())
        if got == 0:
            assert lib.kq_same_get_slot(h, 0, C.byref(out)) == 0 and 8 <= out.W <= 32
        assert lib.kq_same_destroy(h) == 0
    for low in (24000.0, 12000.0):
        h = lib.kq_same_create(C.byref(_cfg(samprate=low, block_len=8)))
        assert lib.kq_same_set(h, 0, C.byref(same_params())) == -1 and b"outside 2048..8192" in lib.kq_last_error()
        assert lib.kq_same_destroy(h) == 0


@pytest.mark.parametrize("Fs,B", [(48000.0, 8), (48000.0, 11), (39062.5, 8), (96000.0, 23)])
def test_table_and_slot_match_the_model(lib, Fs, B):
    """C, inc_m, inc_s, tb and W are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_same_create(C.byref(_cfg(samprate=Fs, block_len=B)))
    assert h, lib.kq_last_error()
    tab = np.zeros(sm.TABLE + 2, np.int16)
    assert lib.kq_same_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()        # cap is kept
    assert lib.kq_same_get_table(h, tab.ctypes.data, sm.TABLE + 2) == 1024 and not tab[sm.TABLE:].any()
    assert np.array_equal(tab[:sm.TABLE], sm.cos_table())
    out = SameSlot()
    lo, hi = Fs / (B * 32.0), Fs / (B * 8.0)                          # the baud rates the geometry takes
    bauds = [b for b in (300.0, sm.BAUD, 520.83, 600.0, 1200.0, lo * 1.001, hi * 0.999) if lo * 1.001 <= b <= hi * 0.999]
    assert len(bauds) >= 3
    for slot, baud in enumerate(bauds[:8]):
        mark, space = (sm.MARK, 0.001, 1234.567, Fs / 2 - 1.0)[slot % 4], (sm.SPACE, 399.99, 3141.59, 50.0)[slot % 4]
        assert lib.kq_same_set(h, slot, C.byref(same_params(slot, mark, space, baud))) == 0, lib.kq_last_error()
        assert lib.kq_same_get_slot(h, slot, C.byref(out)) == 0
        tb = sm.bit_length(Fs, B, baud)
        assert (out.inc_m, out.inc_s, out.tb, out.W) == (sm.same_inc(mark, Fs), sm.same_inc(space, Fs), tb, sm.window(tb)), baud
        assert 8 <= out.W <= 32
    assert lib.kq_same_remove(h, 2) == 0 and lib.kq_same_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_same_destroy(h) == 0
