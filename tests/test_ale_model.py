"""The ALE integer model (tests/ale_model.py) and the protocol helpers (ka9q_sdr_amd/ale2g.py) on the CPU: the Golay code is
what the header says it is; every word survives the way out and back; a call decodes to its addresses; the events do not
depend on how the stream is cut; 100 ppm of clock offset lose nothing; under white noise every word is read at 20 and 14 dB
and the loss further down is printed; noise alone and a steady carrier file nothing, with the gate and with the gate held
open.  tests/test_gpu_ale.py holds the kernel equal to this model bit for bit, so what is shown here holds for the bank.

Measured with this file (the model on a CPU, snr 80, acq_err 1, four runs of 16 random words behind four lead-in words,
white noise; payload words read of 64, printed by the two noise tests below and copied into include/ka9q_hip.h and DESIGN
4.26): 64 at 20, 14, 12, 10 and 8 dB Es/N0 at (8000, 8) and at (39062.5, 32); 27 and 32 at 6 dB, one word read wrong at
each.  Noise alone: 16 sig / nse from 56.0 to 81.5, mean 66.4, the gate open at 101 of 7497 symbols."""
import collections
import functools
import itertools

import numpy as np
import pytest

import ale_model as am
from ka9q_sdr_amd import ale2g

AMP = 0.1
GEOMETRIES = [(8000.0, 8), (39062.5, 32)]


def test_golay_weight_distribution_and_syndromes():
    w = collections.Counter(bin(ale2g.golay_encode(d)).count("1") for d in range(4096))
    assert dict(w) == {0: 1, 8: 759, 12: 2576, 16: 759, 24: 1}
    assert len(ale2g.golay_parity()) == 4096 and int(ale2g.PARITY.max()) < 4096
    assert int((ale2g.ERRORS >> 12 < 4).sum()) == 2325 == 1 + 24 + 276 + 2024      # distinct syndromes, every one of them
    # linear: the check bits of a sum are the sum of the check bits
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 4096, 500), rng.integers(0, 4096, 500)
    assert np.array_equal(ale2g.PARITY[a] ^ ale2g.PARITY[b], ale2g.PARITY[a ^ b])


def test_golay_corrects_three_and_reports_four():
    rng = np.random.default_rng(2)
    for n in range(4):
        for places in itertools.combinations(range(24), n):
            e = sum(1 << p for p in places)
            for d in rng.integers(0, 4096, 3 if n == 3 else 8):
                assert ale2g.golay_decode(ale2g.golay_encode(int(d)) ^ e) == (int(d), n), (d, places)
    for places in itertools.combinations(range(24), 4):
        e = sum(1 << p for p in places)
        d = int(rng.integers(0, 4096))
        c = ale2g.golay_encode(d) ^ e
        assert ale2g.golay_decode(c) == (c >> 12, 4), (d, places)


def _through_register(symbols):
    """the tones shifted into a 147-bit register as the header's step 3 does"""
    r = [0, 0, 0]
    for s in symbols:
        g = ale2g.GRAY[int(s)]
        r = [(r[0] << 3 | r[1] >> 46) & am.M49, (r[1] << 3 | r[2] >> 46) & am.M49, (r[2] << 3 | g) & am.M49]
    return r


def test_every_word_round_trips():
    """every preamble, and all 38^3 character triples (the preambles in turn), through word_bits and the word attempt; and
    every preamble with 300 triples through word_symbols and the register as well"""
    cs = ale2g.CHARSET
    for k, (a, b, c) in enumerate(itertools.product(cs, cs, cs)):
        w = ale2g.word(k % 8, a + b + c)
        v = ale2g.word_bits(w)
        assert am.attempt(v, v, v) == (w, 0, 0, 0, 0) and am.address_like(w)
    assert k + 1 == 38 ** 3
    rng = np.random.default_rng(3)
    for k in range(300):
        chars = "".join(cs[int(i)] for i in rng.integers(0, 38, 3)) if k % 8 != ale2g.CMD else "".join(chr(int(i)) for i in rng.integers(0, 128, 3))
        w = ale2g.word(k % 8, chars)
        sym = ale2g.word_symbols([w])
        assert len(sym) == 49 and am.attempt(*_through_register(sym)) == (w, 0, 0, 0, 0)
        assert ale2g.unword(w) == (ale2g.PREAMBLES[k % 8], chars)
    assert not am.address_like(ale2g.word("TO", "ab1")) and am.address_like(ale2g.word("CMD", "ab1"))


def test_addresses_and_reader():
    assert ale2g.address_words("TO", "ABCDE") == [ale2g.word("TO", "ABC"), ale2g.word("DATA", "DE@")]
    assert [ale2g.unword(w)[0] for w in ale2g.address_words("TIS", "ABCDEFGHIJ")] == ["TIS", "DATA", "REP", "DATA"]
    with pytest.raises(ValueError):
        ale2g.address_words("TO", "ab-")
    call = ale2g.individual_call("K1ABC", "W1AW", scans=2)
    E = collections.namedtuple("E", "word flags")
    assert ale2g.read([E(w, 0) for w in call]) == [("TO", "K1A"), ("TO", "K1A"), ("TO", "K1ABC"), ("TO", "K1ABC"), ("TIS", "W1AW")]
    holed = [E(w, int(k == 3)) for k, w in enumerate(call)]
    assert ale2g.read(holed)[2] == ("TO", "K1A" + ale2g.REPLACEMENT * 3)
    assert ale2g.ale_config(12000.0) == dict(block_len=12) and ale2g.ale_config(8000.0) == dict(block_len=8)


@pytest.mark.parametrize("Fs,B", GEOMETRIES + [(12000.0, 12), (48000.0, 24)])
def test_an_individual_call_decodes_to_its_addresses(Fs, B):
    call = ale2g.individual_call("K1ABC", "W1AW", scans=2)
    m = am.AleModel(Fs, B).feed(ale2g.modulate(call, Fs, amp=AMP, lead=30, tail=10))
    assert [e.word for e in m.events] == call and not any(e.flags or e.err_a or e.err_b or e.split for e in m.events)
    assert ale2g.read(m.events)[-3:] == [("TO", "K1ABC"), ("TO", "K1ABC"), ("TIS", "W1AW")]
    assert np.all(np.abs(np.diff([e.end_sample for e in m.events]) - 0.392 * Fs) <= 2 * B)    # the clock steps by frames


def test_call_boundaries_change_nothing():
    Fs, B = 8000.0, 8
    x = ale2g.modulate(ale2g.individual_call("ABC", "XYZ"), Fs, amp=AMP, lead=12, tail=6)
    x = x + np.random.default_rng(4).normal(0.0, am.noise_sigma(AMP, 14.0, Fs), len(x)).astype(np.float32)
    whole = am.AleModel(Fs, B).feed(x)
    assert len(whole.events) == 4
    for cut in (1, B - 1, B, B + 1, 9000):
        m = am.AleModel(Fs, B)
        for at in range(0, len(x), cut):
            m.feed(x[at:at + cut])
        assert m.events == whole.events and m.status() == whole.status(), cut


@pytest.mark.parametrize("ppm", [100.0, -100.0])
def test_clock_offset_loses_nothing(ppm):
    Fs, B = 8000.0, 8
    rng = np.random.default_rng(5)
    words = [ale2g.word("TO", "ABC")] + [ale2g.word("DATA", "".join(ale2g.CHARSET[int(i)] for i in rng.integers(0, 38, 3)))
                                         for _ in range(19)]
    m = am.AleModel(Fs, B).feed(ale2g.modulate(words, Fs, amp=AMP, lead=30, tail=10, ppm=ppm))
    assert [e.word for e in m.events] == words and not any(e.flags for e in m.events)


def _traffic(seed):
    rng = np.random.default_rng(seed)
    pre = ("DATA", "THRU", "TO", "TWAS", "FROM", "TIS", "REP")
    return [ale2g.word("TO", "ABC")] * 4, [ale2g.word(pre[int(rng.integers(0, 7))], "".join(ale2g.CHARSET[int(i)] for i in rng.integers(0, 38, 3)))
                                           for _ in range(16)]


@functools.lru_cache(maxsize=None)
def _read_under_noise(Fs, B, db):
    """payload words read (of 64) in four runs of 16 random words behind four lead-in words, and words filed that were
    not sent"""
    read = wrong = 0
    for seed in range(4):
        lead, pay = _traffic(seed)
        x = ale2g.modulate(lead + pay, Fs, amp=AMP, lead=40, tail=20)
        x = x + np.random.default_rng(100 + seed).normal(0.0, am.noise_sigma(AMP, db, Fs), len(x)).astype(np.float32)
        got = [e.word for e in am.AleModel(Fs, B).feed(x).events if not e.flags]
        read += sum(1 for w in pay if w in got)
        wrong += sum(1 for w in got if w not in lead + pay)
    return read, wrong


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
@pytest.mark.parametrize("db", [20, 14])
def test_every_word_is_read_at_20_and_14_db(Fs, B, db):
    read, wrong = _read_under_noise(Fs, B, db)
    print("ale noise", Fs, B, db, "dB:", read, "of 64 read,", wrong, "filed that were not sent")
    assert read == 64 and wrong == 0


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
def test_loss_further_down_is_measured(Fs, B):
    """not asserted beyond the arithmetic: printed, and copied into the module's docstring, the header comment and DESIGN
    4.26"""
    for db in (12, 10, 8, 6):
        read, wrong = _read_under_noise(Fs, B, db)
        print("ale noise", Fs, B, db, "dB:", read, "of 64 read,", wrong, "filed that were not sent")
        assert 0 <= read <= 64


@pytest.mark.parametrize("gate", [True, False])
def test_noise_alone_files_nothing(gate):
    """60 s of white noise at amplitude 0.1: with the gate, and by the code and the character test alone"""
    Fs, B = 8000.0, 8
    x = np.random.default_rng(6).normal(0.0, 0.1, int(60 * Fs)).astype(np.float32)
    m = am.AleModel(Fs, B, gate=gate)
    ratio = []
    for at in range(0, len(x), 8000):
        m.feed(x[at:at + 8000])
        if at >= 16000:
            ratio.append(16.0 * m.sig / m.nse)
    print("ale noise alone, gate", gate, ": 16 sig / nse from %.1f to %.1f, mean %.1f; symbols valid %d of %d"
          % (min(ratio), max(ratio), np.mean(ratio), sum(v for _, v in m.syms), len(m.syms)))
    assert not m.events and m.nevents == 0
    assert gate or all(v for _, v in m.syms)


@pytest.mark.parametrize("gate", [True, False])
def test_a_steady_carrier_files_nothing(gate):
    """20 s of tone 2 alone: the gate is wide open on it either way; all-equal tribits are no codeword"""
    Fs, B = 8000.0, 8
    x = ale2g.modulate_symbols([2] * 2500, Fs, amp=AMP, lead=0, tail=0)
    m = am.AleModel(Fs, B, gate=gate).feed(x)
    assert sum(v for _, v in m.syms) > 2400 and {s for s, _ in m.syms[10:]} == {2}
    assert not m.events and m.nevents == 0


def test_a_full_arena_counts_what_it_drops():
    Fs, B = 8000.0, 8
    call = ale2g.individual_call("K1ABC", "W1AW", scans=2)
    m = am.AleModel(Fs, B, max_events=3).feed(ale2g.modulate(call, Fs, amp=AMP, lead=30, tail=10))
    assert len(m.events) == 3 and m.nevents == len(call) and m.dropped == len(call) - 3


def test_widest_intermediates_stay_inside_the_header_bounds():
    """a full-scale square wave at B = 256, W = 32: the header's bounds on the frame sums, the reduced sums, the window
    sums, the powers and oth"""
    Fs, B = 1024000.0, 256
    n = np.arange(40 * 8192)
    x = np.sign(np.cos(2 * np.pi * 1250.0 / Fs * n)).astype(np.float32)
    m = am.AleModel(Fs, B).feed(x)
    assert m.W == 32
    wd = m.widest
    print("ale widest", {k: v.bit_length() for k, v in wd.items()})
    assert wd["acc"] < 1 << 38 and wd["red"] <= (1 << 26) + 2 and wd["sum"] < 1 << 31 and wd["P"] < 1 << 63 and wd["oth"] < 1 << 63
    assert wd["P"] > 1 << 58
