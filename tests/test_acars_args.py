"""Argument checks of the ACARS decoder bank (kq_acars_*): every limit is refused with -1 / NULL and a reason that names the
function and the field before any HIP call, so they hold without a GPU (kq_acars_create, kq_acars_set and kq_acars_remove
touch no device: the next call does); and the taps and the integers the bank makes of a sample rate against the
model's."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import acars_model as am
import ka9q_sdr_amd as kq
from ka9q_sdr_amd.acars import INFO_DTYPE, STATUS_DTYPE, STATUS_WORDS, AcarsConfig, AcarsParams, AcarsSlot, _bind, acars_params


def _slot_checks(lib, bank):
    """no slot is set yet; a set slot reads back; the getters' own refusals"""
    out = AcarsSlot()
    assert lib.kq_acars_get_slot(bank, 0, C.byref(out)) == -1
    assert b"slot 0 holds no decoder" in lib.kq_last_error()
    assert lib.kq_acars_set(bank, 1, C.byref(acars_params(5))) == 0, lib.kq_last_error()
    assert lib.kq_acars_get_slot(bank, 1, C.byref(out)) == 0 and out.source == 5
    assert lib.kq_acars_get_slot(bank, 8, C.byref(out)) == -1 and lib.kq_acars_get_slot(bank, 1, None) == -1
    assert lib.kq_last_error() == b"kq_acars_get_slot: null out"
    assert lib.kq_acars_get_taps(bank, None, 4) == -1
    assert lib.kq_last_error() == b"kq_acars_get_taps: null dst"
    assert lib.kq_acars_remove(bank, 1) == 0


BLOCK, INFO = np.zeros(256, np.uint8), np.zeros(1, INFO_DTYPE)
SUITE = bank_args.Suite(
    "acars", AcarsConfig, acars_params, _bind, status=STATUS_DTYPE, record="block", pull=(BLOCK.ctypes.data, 256, INFO.ctypes.data),
    null_pull=b"null dst", slot_limit=4096,
    default=dict(device=0, samprate=12000.0, input_scale=32767.0, sync_num=1, sync_den=2, max_parity_errors=3, max_block_bytes=256,
                 max_slots=8, max_blocks=4, max_samples=1 << 14, stream=None),
    bad_configs=[
        (dict(samprate=0.0), b"samprate 0 must be positive and finite"),
        (dict(samprate=float("nan")), b"samprate nan"),
        (dict(samprate=float("inf")), b"samprate inf"),
        (dict(samprate=9599.0), b"samprate 9599 must be 9600..96000"),
        (dict(samprate=96000.5), b"samprate 96000.5 must be 9600..96000"),
        (dict(samprate=-12000.0), b"samprate -12000"),
        (dict(input_scale=0.0), b"input_scale"),
        (dict(input_scale=-1.0), b"input_scale"),
        (dict(input_scale=float("nan")), b"input_scale"),
        (dict(input_scale=float("inf")), b"input_scale"),
        (dict(sync_den=0), b"sync_den 0 must be 1..255"),
        (dict(sync_den=256), b"sync_den 256 must be 1..255"),
        (dict(sync_num=0), b"sync_num 0 must be 1..2"),
        (dict(sync_num=3), b"sync_num 3 must be 1..2"),
        (dict(max_parity_errors=256), b"max_parity_errors 256 must be 0..255"),
        (dict(max_block_bytes=15), b"max_block_bytes 15 must be 16..256"),
        (dict(max_block_bytes=257), b"max_block_bytes 257 must be 16..256"),
        (dict(max_slots=0), b"max_slots 0 must be 1..4096"),
        (dict(max_slots=4097), b"max_slots 4097"),
        (dict(max_blocks=0), b"max_blocks 0 must be 1..4096"),
        (dict(max_blocks=4097), b"max_blocks 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
    ],
    more_slot_checks=_slot_checks,
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_blocks", ()), ("pull_counts", (None,)),
                  ("get_taps", (None, 0)), ("get_slot", (0, None)), ("pull_block", (0, 0, None, 0, None))],
    first_call=dict(bank=kq.AcarsBank, geometry=(12000.0,), set=dict(source=3), read=lambda b: b.get_slot(0).source, want=3,
                    again=dict(source=0), refused=[((8000.0,), {}, "samprate 8000 must be 9600..96000")]))
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_and_params_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot
test_set_needs_no_device_and_the_first_call_says_where_there_is_none = SUITE.first_call


NAMES = {"kq_acars_create", "kq_acars_destroy", "kq_acars_set", "kq_acars_remove", "kq_acars_process", "kq_acars_pull_counts",
         "kq_acars_pull_block", "kq_acars_clear_blocks", "kq_acars_get_taps", "kq_acars_get_slot", "kq_acars_sync",
         "kq_acars_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_acars_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.AcarsBank and kq.AcarsParams and kq.acars_params and kq.acars.status_array and kq.acars.INFO_DTYPE
    for n in ("parity", "crc", "encode_block", "modulate", "parse", "repair", "read_blocks"):
        assert callable(getattr(kq.arinc618, n)), n


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 120 and STATUS_WORDS == 30 and INFO_DTYPE.itemsize == 56
    f = STATUS_DTYPE.fields
    assert f["dropped"][1] == 16 and f["in_block"][1] == 24 and f["nbits"][1] == 32 and f["crc"][1] == 48 and f["cnt"][1] == 56
    assert f["t"][1] == 64 and f["search_from"][1] == 72 and f["acc"][1] == 80 and f["sync_sample"][1] == 88
    assert f["sync_c2"][1] == 96 and f["sync_e"][1] == 104 and f["rr"][1] == 112 and f["ri"][1] == 116
    g = INFO_DTYPE.fields
    assert g["flags"][1] == 4 and g["parity_errors"][1] == 8 and g["sync_sample"][1] == 16 and g["end_sample"][1] == 24
    assert g["sync_c2"][1] == 32 and g["sync_e"][1] == 40 and g["r2"][1] == 48
    assert C.sizeof(AcarsParams) == 4 and C.sizeof(AcarsConfig) == 64 and C.sizeof(AcarsSlot) == 32
    assert AcarsConfig.samprate.offset == 8 and AcarsConfig.input_scale.offset == 16 and AcarsConfig.sync_num.offset == 20
    assert AcarsConfig.max_block_bytes.offset == 32 and AcarsConfig.max_blocks.offset == 40
    assert AcarsConfig.max_samples.offset == 48 and AcarsConfig.stream.offset == 56
    assert tuple(STATUS_DTYPE.names) == am.STATUS
    assert (kq.acars.GOOD, kq.acars.ENDED_BY_ETB, kq.acars.OVERRUN) == (am.GOOD, am.BY_ETB, am.OVERRUN) == (1, 2, 4)
    assert kq.arinc618.Record._fields == am.Record._fields


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    for kw in (dict(), dict(samprate=9600.0), dict(samprate=96000.0), dict(samprate=39062.5), dict(sync_num=255, sync_den=255),
               dict(sync_den=1), dict(max_parity_errors=0), dict(max_parity_errors=255), dict(max_block_bytes=16),
               dict(max_slots=4096, max_blocks=1), dict(max_blocks=4096), dict(max_samples=1), dict(max_samples=1 << 28)):
        h = lib.kq_acars_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_acars_destroy(h) == 0


@pytest.mark.parametrize("Fs", [9600.0, 12000.0, 16000.0, 22050.0, 39062.5, 48000.0, 96000.0])
def test_taps_and_integers_match_the_model(lib, Fs):
    """hq, inc, FL, w, e, tb and H are the model's, to the last bit: one cosine or one division in double each; and the
    kernel's piece leaves its workgroup inside 64 KiB of LDS"""
    h = lib.kq_acars_create(C.byref(_cfg(samprate=Fs)))
    assert h, lib.kq_last_error()
    g = am.Geom(Fs)
    taps = np.zeros(82, np.int16)
    assert lib.kq_acars_get_taps(h, taps.ctypes.data, 2) == g.FL and not taps[2:].any()            # cap is kept
    assert lib.kq_acars_get_taps(h, taps.ctypes.data, 82) == g.FL and not taps[g.FL:].any()
    assert np.array_equal(taps[:g.FL], g.hq) and np.array_equal(g.hq, g.hq[::-1])
    out = AcarsSlot()
    assert lib.kq_acars_set(h, 2, C.byref(acars_params(9))) == 0
    assert lib.kq_acars_get_slot(h, 2, C.byref(out)) == 0
    assert (out.source, out.inc, out.taps, out.w, out.e, out.tb, out.history) == (9, g.inc, g.FL, g.w, g.e, g.tb, g.H)
    assert 8 <= g.FL <= 80 and 4 <= g.w <= 40 and 1 <= g.e <= 10 and g.e <= g.w and g.H <= 1719 and g.off[39] == 0
    assert out.piece in (64, 128, 256)
    waves = 4 if Fs < 96000.0 else 2
    words = 512 + 40 + 20 + waves * ((out.piece + g.FL - 1) + (g.HA + out.piece) + (2 * g.w + out.piece) + out.piece // 64)
    assert 8 * words <= 65536
    assert lib.kq_acars_remove(h, 2) == 0 and lib.kq_acars_get_slot(h, 2, C.byref(out)) == -1
    assert lib.kq_acars_destroy(h) == 0
