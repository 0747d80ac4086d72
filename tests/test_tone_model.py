"""The model of the tone signalling decoder (tests/tone_model.py, the header's kq_tone_* comment in numpy and Python ints) on
its own, without a GPU: it decodes every key of seeded DTMF trains with frequency error, twist and noise, and five-tone ZVEI1
calls; it finds nothing in noise; no sum or compare leaves 64 bits at the limits; and any split of a stream into calls
gives the same output.  The GPU tests hold the bank equal to this model bit for bit."""
import numpy as np
import pytest

import tone_model as tm
from ka9q_sdr_amd import selcall as sc


_dtmf_train = tm.dtmf_train


@pytest.mark.parametrize("Fs,B", [(8000.0, 102), (48000.0, 612)])
def test_dtmf_trains_decode(Fs, B):
    cfg = sc.plan_config(sc.DTMF, Fs)
    assert cfg["block_len"] == B and cfg["frac"] == 16
    for k in range(20):
        keys, lead, x = _dtmf_train(Fs, B, 1000 + k, (-4.0, 0.0, 4.0)[k % 3])
        m = tm.ToneModel(Fs, **cfg).feed(x)
        got = sc.read_dtmf(m.events, B)
        assert "".join(g.key for g in got) == keys, (Fs, k, keys, got)
        for i, g in enumerate(got):                          # the key's first whole block begins within a block of its start
            at = (lead + 0.1 * i) * Fs
            assert at - B <= g.start_sample <= at + B and 2 <= g.blocks <= 4, (k, i, g, at)


@pytest.mark.parametrize("Fs,B", [(8000.0, 140), (39062.5, 500)])
def test_five_tone_calls_decode(Fs, B):
    cfg = sc.plan_config(sc.ZVEI1, Fs, block_len=B)
    assert sc.plan_config(sc.ZVEI1, 8000.0)["block_len"] == 140 and cfg["frac"] == 64 and cfg["groups"] == (11,)
    for k in range(20):
        digits, lead, x = tm.zvei_train(Fs, B, k)
        m = tm.ToneModel(Fs, **cfg).feed(x)
        calls = sc.read_sequence(m.events, B, sc.ZVEI1)
        assert [c.digits for c in calls] == [digits], (k, digits, calls, m.events)
        assert abs(calls[0].start_sample - lead * Fs) <= B
    assert sc.sequence_keys("11211", sc.ZVEI1) == "1E21E" and sc.sequence_keys("111", sc.ZVEI1) == "1E1"


def test_noise_gives_no_valid_block():
    Fs = 8000.0
    x = np.random.default_rng(3).normal(0.0, 0.1, int(120 * Fs)).astype(np.float32)
    m = tm.ToneModel(Fs, **sc.plan_config(sc.DTMF, Fs)).feed(x)
    assert m.blocks == 9411 and m.valid == 0 and not m.events and m.cur == -1


def test_sums_stay_inside_64_bits():
    """q = +-32767 in phase with the tone over B = 4096: the largest |I|, P and R there can be"""
    Fs, B = 48000.0, 4096
    m = tm.ToneModel(Fs, B, [1000.0], (1,), frac=128, ratio=4095, twist=4095, min_ms=0xFFFFFFFF)
    n = np.arange(2 * B, dtype=np.uint64)
    j = ((n * np.uint64(m.incs[0])) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)
    q = np.where(m.C[j.astype(np.int64)] >= 0, 32767, -32768).astype(np.int16)      # -32768 reads as -32767
    I, Q, E = tm.block_sums(tm.fm.quantise(q[:B], 1.0, s16=True), 0, m.incs, m.C)
    assert E == B * 32767 ** 2 and 2 ** 41 < I[0] < 2 ** 42 and abs(Q[0]) < 2 ** 42
    P = tm.powers(I, Q)
    assert 2 ** 52 < P[0] < 2 ** 55 and E * B < 2 ** 54
    m.feed(q, s16=True)
    assert m.blocks == 2 and max(m.widest) < 2 ** 63 and m.status()["energy"] == E
    assert m.valid == 0                                      # min_ms at its largest: 2^32 - 1 > 32767^2
    # a square wave's fundamental holds 8 / pi^2 of its power: P = 0.405 R, frac 103 of the pure tone's 128
    m = tm.ToneModel(Fs, B, [1000.0], (1,), frac=100, min_ms=32767 ** 2).feed(q, s16=True)
    assert m.valid == 2 and m.cur == 0 and m.run == 2
    assert tm.ToneModel(Fs, B, [1000.0], (1,), frac=108, min_ms=0).feed(q, s16=True).valid == 0


def test_compares_stay_inside_uint64_at_the_limits():
    """the bounds of the header (P < 2^55, E <= 2^30 B, B <= 4096) through the decision at the largest frac, ratio, twist"""
    B, E, Pmax = 4096, 4096 * 32767 ** 2, 2 ** 55 - 1
    for groups, P in (((1,), [Pmax]), ((2,), [Pmax, Pmax]), ((2, 2), [Pmax] * 4), ((1, 1), [Pmax, Pmax - 1])):
        seen = []
        s = tm.decide(P, E, B, groups, 0xFFFFFFFF, 128, 4095, 4095, seen)
        assert max(seen) < 2 ** 64 and min(seen) >= 0, (groups, max(seen).bit_length())
        assert s == -1                                       # E < min_ms B
    assert tm.decide([Pmax], E, B, (1,), 0, 128, 4095, 4095) == 0
    assert tm.decide([Pmax, Pmax], E, B, (2,), 0, 128, 16, 16) == 0            # ties: the lowest index, ratio 1
    assert tm.decide([Pmax, Pmax], E, B, (2,), 0, 128, 17, 16) == -1
    assert tm.decide([5 << 40, 9 << 40, 1 << 50, 3 << 40], 1 << 30, 64, (2, 2), 16, 16, 64, 160) == -1    # twist
    assert tm.decide([5 << 40, 9 << 48, 1 << 50, 3 << 40], 1 << 30, 64, (2, 2), 16, 16, 64, 160) == 1
    assert tm.decide([5 << 40, 1 << 50, 3 << 40, 9 << 48], 1 << 30, 64, (2, 2), 16, 16, 64, 160) == 1 | 1 << 8


def test_any_split_into_calls_gives_the_same_output():
    Fs, B = 8000.0, 102
    cfg = sc.plan_config(sc.DTMF, Fs)
    keys, _, x = _dtmf_train(Fs, B, 5, 0.0)
    whole = tm.ToneModel(Fs, **cfg).feed(x)
    assert "".join(g.key for g in sc.read_dtmf(whole.events, B)) == keys
    rng = np.random.default_rng(9)
    for sizes in ((1, 63, 64, 65, B - 1, B, B + 1, 1000, 7777), tuple(int(v) for v in rng.integers(1, 400, 50))):
        m, at, k = tm.ToneModel(Fs, **cfg), 0, 0
        while at < len(x):
            m.feed(x[at:at + sizes[k % len(sizes)]])
            at += sizes[k % len(sizes)]
            k += 1
        assert m.events == whole.events and m.status() == whole.status() and m.powers() == whole.powers()
        assert m.symbols == whole.symbols and m.I == whole.I and m.E == whole.E


def test_a_slot_set_in_mid_block_sees_zeros_before_it():
    Fs, B = 8000.0, 102
    cfg = sc.plan_config(sc.DTMF, Fs)
    _, _, x = _dtmf_train(Fs, B, 6, 0.0)
    late = tm.ToneModel(Fs, start=150, **cfg).feed(x[150:])
    zeroed = tm.ToneModel(Fs, **cfg).feed(np.concatenate([np.zeros(150, np.float32), x[150:]]))
    assert late.events == zeroed.events and late.powers() == zeroed.powers() and late.blocks == zeroed.blocks - 1
