"""Argument checks of the POCSAG pager decoder bank (kq_pag_*): every limit is refused with -1 / NULL and a reason that names
the function and the field before any HIP call, so they hold without a GPU (kq_pag_create touches no device); the
quantised low-pass the bank designs against the model's own design; and kq_pag_correct, the host's view of the
correction table the device gets, over every pattern of up to two errors and a sample of those with three."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bank_args
import ka9q_sdr_amd as kq
import fsk_model as fm
import pag_model as pm
from ka9q_sdr_amd.pag import INFO_DTYPE, STATUS_DTYPE, STATUS_WORDS, PagConfig, PagParams, _bind, correct, pag_params


PAGE = np.zeros(64, np.uint8)
SUITE = bank_args.Suite(
    "pag", PagConfig, pag_params, _bind, status=STATUS_DTYPE, record="page", pull=(PAGE.ctypes.data, 64, None), null_pull=b"null dst",
    slot_limit=4096, set_needs_device=True,
    default=dict(device=0, samprate=19200.0, baud=1200, taps=31, cutoff_hz=900.0, kaiser_beta=2.0, window_bits=24.0,
                 input_scale=4096.0, pll_shift=3, max_slots=8, max_pages=4, max_page_words=16, max_samples=1 << 14, stream=None),
    bad_configs=[
        (dict(samprate=4799.0), b"samprate 4799 must be 4 .. 40 times baud 1200"),
        (dict(samprate=48000.5), b"samprate 48000.5 must be 4 .. 40 times baud 1200"),
        (dict(samprate=39062.5, baud=512, cutoff_hz=384.0), b"samprate 39062.5 must be 4 .. 40 times baud 512"),   # via kq_rsmp_*
        (dict(samprate=3000.0), b"samprate 3000"),                         # 2.5 samples per bit
        (dict(baud=0), b"baud 0"),
        (dict(baud=-1200), b"baud -1200"),
        (dict(samprate=-1.0), b"samprate -1"),
        (dict(samprate=0.0), b"samprate 0"),
        (dict(samprate=float("nan")), b"samprate nan"),
        (dict(samprate=float("inf")), b"samprate inf"),
        (dict(taps=30), b"taps 30 must be odd"),
        (dict(taps=1), b"taps 1"),
        (dict(taps=129), b"taps 129"),
        (dict(window_bits=0.05), b"window_bits 0.05 gives W = 1 samples"),
        (dict(window_bits=64.1), b"gives W = 1026 samples"),
        (dict(samprate=48000.0, window_bits=25.7), b"gives W = 1028 samples"),
        (dict(window_bits=float("nan")), b"window_bits"),
        (dict(window_bits=-4.0), b"window_bits"),
        (dict(cutoff_hz=0.0), b"cutoff_hz 0"),
        (dict(cutoff_hz=9600.0), b"cutoff_hz 9600"),
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
        (dict(max_pages=0), b"max_pages 0"),
        (dict(max_pages=4097), b"max_pages 4097"),
        (dict(max_page_words=0), b"max_page_words 0"),
        (dict(max_page_words=257), b"max_page_words 257"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
        (dict(samprate=4800.0, taps=127, cutoff_hz=720.0), b"> 65535"),   # long filter, four samples per bit: could overflow
    ],
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_pages", ()), ("pull_counts", (None,)),
                  ("get_taps", (None, 0)), ("pull_page", (0, 0, None, 0, None))])
lib, bank, _cfg = SUITE.lib, SUITE.bank, SUITE.cfg
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot


NAMES = {"kq_pag_create", "kq_pag_destroy", "kq_pag_set", "kq_pag_remove", "kq_pag_process", "kq_pag_pull_counts",
         "kq_pag_pull_page", "kq_pag_clear_pages", "kq_pag_get_taps", "kq_pag_sync", "kq_pag_reset", "kq_pag_correct"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_pag_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.PagBank and kq.pag_params and kq.pocsag.encode and kq.pocsag.numeric and kq.pocsag.alpha


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 56 and STATUS_WORDS == 14 and INFO_DTYPE.itemsize == 32
    assert STATUS_DTYPE.fields["pll_phase"][1] == 40 and STATUS_DTYPE.fields["level"][1] == 52
    assert INFO_DTYPE.fields["errors"][1] == 16 and INFO_DTYPE.fields["end_sample"][1] == 24
    assert C.sizeof(PagParams) == 4 and C.sizeof(PagConfig) == 72
    assert PagConfig.samprate.offset == 8 and PagConfig.baud.offset == 16
    assert PagConfig.max_samples.offset == 56 and PagConfig.stream.offset == 64


def test_good_configs_accepted(lib):
    """the limits themselves, and the six geometries of the design; none of them asks for a device"""
    for kw in (dict(), dict(samprate=4800.0), dict(samprate=48000.0, window_bits=25.6),      # Fs = 4 and 40 baud; W = 1024
               dict(samprate=39062.5, baud=2400, cutoff_hz=1800.0), dict(taps=3), dict(taps=127), dict(window_bits=0.125),   # W = 2
               dict(samprate=8192.0, baud=512, cutoff_hz=384.0), dict(pll_shift=1), dict(pll_shift=8),
               dict(max_slots=4096, max_pages=1, max_page_words=1), dict(max_pages=4096, max_page_words=256),
               dict(cutoff_hz=9599.0)):
        h = lib.kq_pag_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_pag_destroy(h) == 0
    for Fs, baud, K, W in pm.CASES:
        h = lib.kq_pag_create(C.byref(_cfg(samprate=Fs, baud=baud, taps=K, cutoff_hz=0.75 * baud,
                                            window_bits=pm.default_window(Fs, baud))))
        assert h, (Fs, baud, K, lib.kq_last_error())
        assert lib.kq_pag_destroy(h) == 0


def test_limits_are_checked_before_any_device_is_asked_for(lib):
    """every refusal above and every acceptance happen in kq_pag_create, which touches no device: with or without a GPU
    in the box a good geometry gives a handle, and what needs a device (the first set) says so where there is none"""
    try:
        b = kq.PagBank(48000.0, 1200, 63, 4, 4096)
        assert b.window_bits == 24.0 and b.cutoff_hz == 900.0
    except kq.KqError as e:
        raise AssertionError("kq_pag_create asked for a device: %s" % e)
    with pytest.raises(kq.KqError, match="samprate 48000 must be 4 .. 40 times baud 512"):
        kq.PagBank(48000.0, 512, 63, 4, 4096)
    try:
        b.set(0, source=0)
        assert lib.kq_device_count() > 0
    except kq.KqError as e:
        assert lib.kq_device_count() <= 0, str(e)
    b.close()


@pytest.mark.parametrize("Fs,baud,K,W", pm.CASES + [(19200.0, 1200, 3, 384), (9600.0, 1200, 127, 192)])
def test_taps_match_the_models_design(lib, Fs, baud, K, W):
    """hq within one LSB of the float64 design of tests/fsk_model.py (i0 and sinc may differ in the last place, and a
    value that close to a half rounds the other way); the GPU tests hand the bank's taps to the model"""
    c = _cfg(samprate=Fs, baud=baud, taps=K, cutoff_hz=0.75 * baud, window_bits=pm.default_window(Fs, baud))
    h = lib.kq_pag_create(C.byref(c))
    assert h, lib.kq_last_error()
    hq = np.zeros(K + 2, np.int16)
    assert lib.kq_pag_get_taps(h, hq.ctypes.data, 2) == K and not hq[2:].any()      # cap is kept
    assert lib.kq_pag_get_taps(h, hq.ctypes.data, K + 2) == K and not hq[K:].any()
    assert lib.kq_pag_destroy(h) == 0
    want = fm.design_taps(K, 0.75 * baud, Fs, 2.0)
    got = hq[:K].astype(np.int64)
    assert np.abs(got - want).max() <= 1 and np.array_equal(got, got[::-1]) and np.abs(got).sum() <= 65535
    assert pm.PagModel(Fs, baud, K).W == W


# ---- the correction table ----
def _codewords():
    rng = np.random.default_rng(17)
    return [pm.FSC, pm.IDLE] + [pm.make_word(int(d)) for d in rng.integers(0, 1 << 21, 64)]


def test_correct_mends_every_pattern_of_up_to_two_errors(lib):
    """66 codewords x (1 + 32 + 496) patterns: the codeword comes back with the number of bits that were wrong"""
    out = C.c_uint32(0)
    pairs = list(itertools.combinations(range(32), 2))
    for w in _codewords():
        assert pm.syndrome(w) == 0 and bin(w).count("1") % 2 == 0
        assert lib.kq_pag_correct(w, C.byref(out)) == 0 and out.value == w
        for i in range(32):
            assert lib.kq_pag_correct(w ^ 1 << i, C.byref(out)) == 1 and out.value == w, (hex(w), i)
        for i, j in pairs:
            assert lib.kq_pag_correct(w ^ 1 << i ^ 1 << j, C.byref(out)) == 2 and out.value == w, (hex(w), i, j)
    assert lib.kq_pag_correct(pm.FSC ^ 5, None) == 2                   # `fixed` may be NULL
    assert correct(pm.IDLE ^ 1 << 31) == (pm.IDLE, 1) and correct(pm.IDLE ^ 7) == (None, -1)


def test_correct_refuses_three_errors(lib):
    """minimum distance 6: a word three bits from a codeword is at least three from every other, so none of the 4960
    patterns can be mended.  2000 of them, spread over the codewords; `fixed` is left alone"""
    rng = np.random.default_rng(18)
    triples = list(itertools.combinations(range(32), 3))
    assert len(triples) == 4960
    words = _codewords()
    out = C.c_uint32(0xDEADBEEF)
    for k in rng.choice(len(triples), 2000, replace=False):
        i, j, l = triples[k]
        w = words[int(k) % len(words)]
        assert lib.kq_pag_correct(w ^ 1 << i ^ 1 << j ^ 1 << l, C.byref(out)) == -1, (hex(w), i, j, l)
        assert pm.correct(w ^ 1 << i ^ 1 << j ^ 1 << l) == (None, -1)
    assert out.value == 0xDEADBEEF


def test_table_agrees_with_the_models(lib):
    """the library's table (21 shift / xor steps and a lookup) and the model's (long division on bit lists), on random words"""
    rng = np.random.default_rng(19)
    out = C.c_uint32(0)
    for x in rng.integers(0, 1 << 32, 3000, dtype=np.uint64):
        n = lib.kq_pag_correct(int(x), C.byref(out))
        v, e = pm.correct(int(x))
        assert n == e and (e < 0 or out.value == v), hex(int(x))
