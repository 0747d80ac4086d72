"""Argument checks of the tone signalling decoder bank (kq_tone_*): every limit is refused with -1 / NULL and a reason that
names the function and the field before any HIP call, so they hold without a GPU (kq_tone_create touches no device); the
cosine table and the phase increments the bank hands out against the model's; and selcall.py's round trip: encode, model,
reader."""
import ctypes as C

import numpy as np
import pytest

import bank_args
import ka9q_sdr_amd as kq
import tone_model as tm
from ka9q_sdr_amd import selcall as sc
from ka9q_sdr_amd.tone import EVENT_DTYPE, STATUS_DTYPE, STATUS_WORDS, ToneConfig, ToneParams, _bind, tone_params


def _cfg(freqs=sc.DTMF.freqs, **kw):
    """freqs=None: DTMF's counts with a null pointer"""
    f = np.ascontiguousarray(sc.DTMF.freqs if freqs is None else freqs, np.float32)
    c = dict(device=0, samprate=8000.0, block_len=102, ntones=f.size, freqs=f.ctypes.data_as(C.POINTER(C.c_float)), group0=4,
             group1=f.size - 4, min_ms=16, frac=16, ratio=64, twist=160, min_blocks=2, input_scale=32767.0, max_slots=8,
             max_events=4, max_samples=1 << 14, stream=None)
    c.update(kw)
    cfg = ToneConfig(*c.values())
    cfg._keep = f
    if freqs is None:
        cfg.freqs = None
    return cfg


EVENT, POWERS = np.zeros(1, EVENT_DTYPE), np.zeros((8, 9), np.uint64)
SUITE = bank_args.Suite(
    "tone", ToneConfig, tone_params, _bind, status=STATUS_DTYPE, record="event", pull=(EVENT.ctypes.data,), null_pull=b"null event",
    slot_limit=4096, cfg=_cfg, set_needs_device=True,
    process_extra=(None, 0), bad_process=[((POWERS.ctypes.data, 8), b"powers_stride 8 < ntones + 1 = 9")],
    bad_configs=[
        (dict(samprate=0.0), b"samprate 0 must be positive and finite"),
        (dict(samprate=-8000.0), b"samprate -8000"),
        (dict(samprate=float("nan")), b"samprate nan"),
        (dict(samprate=float("inf")), b"samprate inf"),
        (dict(block_len=7), b"block_len 7 must be 8..4096"),
        (dict(block_len=4097), b"block_len 4097 must be 8..4096"),
        (dict(ntones=0, group0=0, group1=0), b"ntones 0 must be 1..32"),
        (dict(freqs=np.linspace(300.0, 3400.0, 33), group0=33, group1=0), b"ntones 33 must be 1..32"),
        (dict(group0=0, group1=8), b"groups of 0 and 8 tones"),
        (dict(group0=4, group1=3), b"groups of 4 and 3 tones"),
        (dict(group0=8, group1=1), b"groups of 8 and 1 tones"),
        (dict(group0=0xFFFFFFFF, group1=9), b"groups of 4294967295 and 9 tones"),
        (dict(freqs=None), b"null freqs"),
        (dict(freqs=[697.0, 0.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0]), b"freqs[1] 0 must be above 0"),
        (dict(freqs=[697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 4000.0]), b"freqs[7] 4000 must be above 0 and below"),
        (dict(freqs=[697.0, 770.0, -852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0]), b"freqs[2] -852"),
        (dict(freqs=[float("nan")] * 8), b"freqs[0] nan"),
        (dict(frac=0), b"frac 0 must be 1..128"),
        (dict(frac=129), b"frac 129 must be 1..128"),
        (dict(ratio=15), b"ratio 15 must be 16..4095"),
        (dict(ratio=4096), b"ratio 4096 must be 16..4095"),
        (dict(twist=15), b"twist 15 must be 16..4095"),
        (dict(twist=4096), b"twist 4096 must be 16..4095"),
        (dict(min_blocks=0), b"min_blocks 0 must be 1..65535"),
        (dict(min_blocks=65536), b"min_blocks 65536 must be 1..65535"),
        (dict(input_scale=0.0), b"input_scale"),
        (dict(input_scale=-1.0), b"input_scale"),
        (dict(input_scale=float("nan")), b"input_scale"),
        (dict(input_scale=float("inf")), b"input_scale"),
        (dict(max_slots=0), b"max_slots 0 must be 1..4096"),
        (dict(max_slots=4097), b"max_slots 4097"),
        (dict(max_events=0), b"max_events 0 must be 1..4096"),
        (dict(max_events=4097), b"max_events 4097"),
        (dict(max_samples=0), b"max_samples 0"),
        (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
    ],
    null_handles=[("destroy", ()), ("sync", ()), ("reset", ()), ("remove", (0,)), ("clear_events", ()), ("pull_counts", (None,)),
                  ("get_table", (None, 0)), ("get_incs", (None, 0)), ("pull_event", (0, 0, None))])
lib, bank = SUITE.lib, SUITE.bank
test_null_config_refused, test_bad_config_refused, test_bad_process_refused = SUITE.null_config, SUITE.bad_config, SUITE.bad_process
test_bad_slot_refused, test_null_handles_refused = SUITE.bad_slot, SUITE.null_handles
test_without_a_slot_nothing_touches_a_device = SUITE.without_a_slot


NAMES = {"kq_tone_create", "kq_tone_destroy", "kq_tone_set", "kq_tone_remove", "kq_tone_process", "kq_tone_pull_counts",
         "kq_tone_pull_event", "kq_tone_clear_events", "kq_tone_get_table", "kq_tone_get_incs", "kq_tone_sync",
         "kq_tone_reset"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_tone_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.ToneBank and kq.ToneParams and kq.tone_params and kq.selcall.dtmf_encode and kq.selcall.read_sequence


def test_record_layouts():
    assert STATUS_DTYPE.itemsize == 32 and STATUS_WORDS == 8 and EVENT_DTYPE.itemsize == 24
    assert STATUS_DTYPE.fields["cur"][1] == 16 and STATUS_DTYPE.fields["energy"][1] == 24
    assert EVENT_DTYPE.fields["start_sample"][1] == 8 and EVENT_DTYPE.fields["peak"][1] == 16
    assert C.sizeof(ToneParams) == 4 and C.sizeof(ToneConfig) == 88
    assert ToneConfig.samprate.offset == 8 and ToneConfig.freqs.offset == 24 and ToneConfig.group0.offset == 32
    assert ToneConfig.input_scale.offset == 60 and ToneConfig.max_samples.offset == 72 and ToneConfig.stream.offset == 80


def test_good_configs_accepted(lib):
    """the limits themselves, and the geometries of the GPU tests; none of them asks for a device"""
    one = dict(freqs=[1000.0], group0=1, group1=0)
    many = dict(freqs=np.linspace(300.0, 3400.0, 32), group0=32, group1=0)
    for kw in (dict(), dict(block_len=8), dict(block_len=4096), one, many, dict(many, group0=1, group1=31),
               dict(samprate=39062.5, block_len=500), dict(samprate=3266.1), dict(freqs=[0.001] * 8), dict(frac=1),
               dict(frac=128), dict(ratio=16), dict(ratio=4095), dict(twist=16), dict(twist=4095), dict(min_blocks=1),
               dict(min_blocks=65535), dict(min_ms=0), dict(min_ms=0xFFFFFFFF), dict(max_slots=4096, max_events=1),
               dict(max_events=4096), dict(max_samples=1), dict(max_samples=1 << 28)):
        h = lib.kq_tone_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_tone_destroy(h) == 0
    for plan, Fs in ((sc.DTMF, 48000.0), (sc.ZVEI1, 39062.5), (sc.CCIR, 8000.0)):
        try:
            kq.ToneBank(Fs, max_slots=4, max_samples=4096, **sc.plan_config(plan, Fs)).close()
        except kq.KqError as e:
            raise AssertionError("%s at %g: %s" % (plan.name, Fs, e))


def test_limits_are_checked_before_any_device_is_asked_for(lib):
    """every refusal above and every acceptance happen in kq_tone_create, which touches no device: with or without a GPU
    in the box a good plan gives a handle, and what needs a device (the first set) says so where there is none"""
    try:
        b = kq.ToneBank(48000.0, max_slots=4, max_samples=4096, **sc.plan_config(sc.DTMF, 48000.0))
        assert b.block_len == 612 and b.frac == 16 and b.groups == (4, 4) and b.ntones == 8
    except kq.KqError as e:
        raise AssertionError("kq_tone_create asked for a device: %s" % e)
    with pytest.raises(kq.KqError, match=r"freqs\[7\] 1633 must be above 0 and below samprate / 2"):
        kq.ToneBank(3000.0, max_slots=4, max_samples=4096, **sc.plan_config(sc.DTMF, 3000.0))
    try:
        b.set(0, source=0)
        assert lib.kq_device_count() > 0
    except kq.KqError as e:
        assert lib.kq_device_count() <= 0, str(e)
    b.close()


@pytest.mark.parametrize("plan,Fs", [(sc.DTMF, 8000.0), (sc.DTMF, 48000.0), (sc.ZVEI1, 39062.5), (sc.CCIR, 19200.0)])
def test_table_and_incs_match_the_model(lib, plan, Fs):
    """C and inc_t are the model's, to the last bit: one cosine and one division in double each"""
    h = lib.kq_tone_create(C.byref(_cfg(freqs=plan.freqs, samprate=Fs, group0=plan.groups[0],
                                        group1=len(plan.freqs) - plan.groups[0])))
    assert h, lib.kq_last_error()
    T = len(plan.freqs)
    tab = np.zeros(tm.TABLE + 2, np.int16)
    assert lib.kq_tone_get_table(h, tab.ctypes.data, 2) == 1024 and not tab[2:].any()        # cap is kept
    assert lib.kq_tone_get_table(h, tab.ctypes.data, tm.TABLE + 2) == 1024 and not tab[tm.TABLE:].any()
    incs = np.zeros(T + 2, np.uint32)
    assert lib.kq_tone_get_incs(h, incs.ctypes.data, 1) == T and not incs[1:].any()
    assert lib.kq_tone_get_incs(h, incs.ctypes.data, T + 2) == T and not incs[T:].any()
    assert lib.kq_tone_destroy(h) == 0
    want = tm.cos_table()
    assert np.array_equal(tab[:tm.TABLE], want)
    assert want[0] == 32767 and want[256] == 0 and want[512] == -32767 and np.array_equal(want[1:], want[:0:-1])
    assert np.array_equal(incs[:T], tm.tone_incs(plan.freqs, Fs))
    assert np.abs(incs[:T].astype(np.float64) * Fs / 2.0 ** 32 - np.asarray(plan.freqs)).max() < Fs / 2.0 ** 32


def test_selcall_round_trips():
    """encode -> model -> reader, for every key of each plan"""
    Fs = 8000.0
    keys = sc.DTMF.keys
    for twist_db in (-4.0, 0.0, 4.0):
        x = sc.dtmf_encode(keys, Fs, twist_db=twist_db, lead=0.02)
        cfg = sc.plan_config(sc.DTMF, Fs)
        got = sc.read_dtmf(tm.ToneModel(Fs, **cfg).feed(x).events, cfg["block_len"])
        assert "".join(g.key for g in got) == keys
        assert all(abs(g.start_sample - (0.02 + 0.1 * i) * Fs) <= cfg["block_len"] for i, g in enumerate(got))
    for plan in (sc.ZVEI1, sc.CCIR):
        cfg = sc.plan_config(plan, Fs)
        assert cfg["block_len"] == int(round(plan.tone_s * Fs / 4))
        x = np.concatenate([sc.sequence_encode(d, Fs, plan, lead=0.1, tail=0.3) for d in ("12345", "67890", "11122", "00700")])
        calls = sc.read_sequence(tm.ToneModel(Fs, **cfg).feed(x).events, cfg["block_len"], plan)
        assert [c.digits for c in calls] == ["12345", "67890", "11122", "00700"]
    assert sc.symbol_key(sc.DTMF, 2 | 3 << 8) == "C" and sc.symbol_key(sc.DTMF, -1) is None
    assert sc.key_tones(sc.DTMF, "#") == (941.0, 1477.0) and sc.key_tones(sc.ZVEI1, "E") == (2600.0,)
    assert sc.symbol_key(sc.ZVEI1, 9) == "0" and sc.symbol_key(sc.ZVEI1, 1 << 8) is None
    # a long key with a block lost in the middle is one key; two keys of one symbol four blocks apart are two
    ev = [tm.Event(1, 3, 1020, 1), tm.Event(1, 4, 1428, 1), tm.Event(1, 2, 2244, 1)]
    assert sc.read_dtmf(ev, 102) == [sc.Key("4", 1020, 8), sc.Key("4", 2244, 2)]
