"""The DSC integer model (tests/dsc_model.py) and the format helpers (ka9q_sdr_amd/itu493.py) on the CPU: the symbol code is
what the header says it is; a sequence puts every symbol where the header says; the three kinds of message survive the way
out, through the register and back; the events do not depend on how the stream is cut; 100 ppm of clock offset lose nothing;
an inverted stream is read and marked; symbols knocked out of the DX copies alone, or of the RX copies alone, are all
rescued; a burst across both copies of one symbol leaves one hole that the host mends; `lose` holes in a row and 64 symbols
without an end each end a message as the header's rules (c) and (b) say; under white noise every message is whole from 20
down to 12 dB and the loss further down is printed; noise alone and a steady tone file nothing, with the gate and with the
gate held open.  tests/test_gpu_dsc.py holds the kernel equal to this model bit for bit, so what is shown here holds for
the bank.

Measured with this file (the model on a CPU, snr 64, acq 2, lose 3; eight individual calls of 23 symbols, each behind 40 bit
times of noise and a 20-bit dot pattern, white noise; messages filed whole with the check good, of 8, printed by the two
noise tests below and copied into include/ka9q_hip.h and DESIGN 4.27): 8 at 20, 14 and 12 dB Es/N0 at (12000, 12) and at
(39062.5, 32); 7 at 10 dB at both (8 once itu493.repair has mended the one hole); 2 and 1 at 8 dB (4 and 4 mended); none at
6 dB.  Noise alone, 240 s: 16 sig / nse from 33.6 to 73.8, mean 48.5, the gate open at 1282 of 23947 bits, no sync taken.
Of 48 starting phases of the clock at 20 dB none is lost with step 1's push, 2 without it."""
import functools

import numpy as np
import pytest

import dsc_model as dm
from ka9q_sdr_amd import itu493 as it

AMP = 0.1
GEOMETRIES = [(12000.0, 12), (39062.5, 32)]
TO, FROM = 232001234, 211239870


def test_the_symbol_code():
    words = [w for w in range(1024) if it.decode_symbol(w) is not None]
    assert len(words) == 128 and sorted(it.decode_symbol(w) for w in words) == list(range(128))
    assert "{:010b}".format(it.encode_symbol(125)) == "1011111001" and dm.W125 == it.encode_symbol(125)
    for v in range(128):
        w = it.encode_symbol(v)
        assert it.decode_symbol(w) == v and dm.is_symbol(w) and dm.value_of(w) == v and dm.word_of(v) == w
        for b in range(10):                                      # every single wrong bit is seen
            assert it.decode_symbol(w ^ 1 << b) is None and not dm.is_symbol(w ^ 1 << b), (v, b)
    assert [dm.is_symbol(w) for w in range(1024)] == [it.decode_symbol(w) is not None for w in range(1024)]
    assert it.decode_symbol(0) is None and it.decode_symbol(1023) is None      # a steady tone is no symbol
    with pytest.raises(ValueError):
        it.encode_symbol(128)


def test_sequence_places():
    sym = it.individual_call(TO, FROM)
    seq = it.sequence(sym)
    n = len(sym)
    assert len(seq) == 2 * n + 16
    assert seq[0:12:2] == [125] * 6 and seq[1:16:2] == list(range(111, 103, -1))
    for i, v in enumerate(sym):
        assert seq[12 + 2 * i] == v and seq[17 + 2 * i] == v, i
    assert sym[0] == sym[1] == 120 and sym[-2] == it.RQ and sym[-1] == it.check_symbol(sym[:-1])
    assert seq[12 + 2 * n] == seq[14 + 2 * n] == it.RQ
    for dots in (20, 200):
        b = it.bits(sym, dots)
        assert len(b) == dots + 10 * len(seq) and b[:4].tolist() == [1, 0, 1, 0]
        assert "".join(map(str, b[dots:dots + 10])) == "1011111001"
    with pytest.raises(ValueError):
        it.bits(sym, 100)
    assert it.dsc_config(12000.0) == dict(block_len=12) and it.dsc_config(96000.0, 1200.0) == dict(block_len=8)
    assert it.dsc_config(48000.0) == dict(block_len=48)
    with pytest.raises(ValueError):
        it.dsc_config(48000.0, 1200.0)


def _through_register(bits, **kw):
    """the bits through the model's steps 3 to 5 alone, the gate held open"""
    m = dm.DscModel(12000.0, 12, gate=False, **kw)
    for k, b in enumerate(bits):
        m.bit = int(b)
        m._bit(k, 0)
    return m


MESSAGES = [("individual", it.individual_call(TO, FROM)), ("individual", it.individual_call(TO, FROM, frequency=(), eos=it.BQ)),
            ("all_ships", it.all_ships(FROM)), ("distress", it.distress_alert(FROM, position="0521301234", time="1359"))]


@pytest.mark.parametrize("kind,sym", MESSAGES, ids=[k + str(len(s)) for k, s in MESSAGES])
@pytest.mark.parametrize("dots", [20, 200])
def test_messages_round_trip_through_the_register(kind, sym, dots):
    m = _through_register(it.bits(sym, dots))
    assert len(m.events) == 1 and m.syncs == 1 and m.aborted == 0 and not m.synced
    e = m.events[0]
    assert (e.nsym, e.flags, e.holes, e.from_rx, e.hole_mask) == (len(sym), 0, 0, 0, 0)
    assert list(e.sym[:e.nsym]) == sym and not any(e.sym[e.nsym:])
    p = it.parse(e)
    assert p["kind"] == kind and p["ok"] and not p["inverted"] and p["symbols"] == sym and p["eos"] == sym[-2]
    assert p["frm"] == "%09d" % FROM
    if kind == "individual":
        assert p["to"] == "%09d" % TO and p["category"] == it.ROUTINE and p["telecommand"] == (it.J3E, it.NO_INFORMATION)
    if kind == "distress":
        assert (p["nature"], p["position"], p["time"], p["telecommand"]) == (it.UNDESIGNATED, "0521301234", "1359", it.J3E)
    assert it.read(m.events) == [p]
    # sync is taken at the first place that shows two of the phasing sequence's other places: v = 110, place 3, whose s2 is
    # 111 and whose s1 and s3 are 125
    assert e.sync_sample == (dots + 40) * 12 and m.place == 17 + 2 * (len(sym) - 1)


@pytest.mark.parametrize("acq,place", [(1, 3), (2, 3), (3, 3)])
def test_sync_place_by_acq(acq, place):
    sym = it.individual_call(TO, FROM, frequency=())
    m = _through_register(it.bits(sym), acq=acq)
    assert len(m.events) == 1 and m.events[0].sync_sample == (20 + 10 * (place + 1)) * 12
    # the dot pattern and place 0 lost: the first attempt that can pass moves by acq
    late = it.bits(sym)[50:]
    m = _through_register(late, acq=acq)
    assert len(m.events) == 1 and list(m.events[0].sym[:len(sym)]) == sym, acq


@pytest.mark.parametrize("Fs,B,baud,mark,space", [(12000.0, 12, 100.0, 1785.0, 1615.0), (12000.0, 8, 100.0, 1785.0, 1615.0),
                                                   (39062.5, 32, 100.0, 1785.0, 1615.0), (48000.0, 56, 100.0, 1785.0, 1615.0),
                                                   (96000.0, 8, 1200.0, 1300.0, 2100.0)])
def test_a_call_decodes_at_every_geometry(Fs, B, baud, mark, space):
    sym = it.individual_call(TO, FROM)
    x = it.modulate(it.bits(sym), Fs, baud, mark, space, amp=AMP, lead=8, tail=8)
    m = dm.DscModel(Fs, B, mark, space, baud).feed(x)
    assert len(m.events) == 1 and it.read(m.events)[0]["symbols"] == sym and m.events[0].flags == 0 and m.events[0].from_rx == 0
    per = Fs / baud
    assert abs(m.events[0].end_sample - m.events[0].sync_sample - 10 * (2 * len(sym) + 12) * per) <= per / 2


def test_call_boundaries_change_nothing():
    Fs, B = 12000.0, 12
    x = it.modulate(it.bits(it.individual_call(TO, FROM, frequency=())), Fs, amp=AMP, lead=12, tail=6)
    x = x + np.random.default_rng(4).normal(0.0, dm.noise_sigma(AMP, 14.0, Fs), len(x)).astype(np.float32)
    whole = dm.DscModel(Fs, B).feed(x)
    assert len(whole.events) == 1 and whole.events[0].flags == 0
    for cut in (1, B - 1, B, B + 1, 9000):
        m = dm.DscModel(Fs, B)
        for at in range(0, len(x), cut):
            m.feed(x[at:at + cut])
        assert m.events == whole.events and m.status() == whole.status(), cut


@pytest.mark.parametrize("ppm", [100.0, -100.0])
def test_clock_offset_loses_nothing(ppm):
    """the longest message there is, 64 symbols, 14.6 s: 100 ppm is 0.15 bit over it"""
    Fs, B = 12000.0, 12
    sym = it.message(it.INDIVIDUAL, list(np.random.default_rng(5).integers(0, 100, 60)))
    assert len(sym) == 64
    m = dm.DscModel(Fs, B).feed(it.modulate(it.bits(sym, 200), Fs, amp=AMP, lead=30, tail=10, ppm=ppm))
    assert len(m.events) == 1 and list(m.events[0].sym) == sym and m.events[0].flags == 0 and m.events[0].from_rx == 0


def test_an_inverted_stream_is_read_and_marked():
    Fs, B = 12000.0, 12
    sym = it.all_ships(FROM)
    x = it.modulate(it.bits(sym), Fs, mark=it.SPACE, space=it.MARK, amp=AMP, lead=8, tail=8)
    m = dm.DscModel(Fs, B).feed(x)
    assert len(m.events) == 1 and m.events[0].flags == it.INVERTED and m.inverted == 1
    p = it.parse(m.events[0])
    assert p["inverted"] and p["ok"] and p["symbols"] == sym
    m = _through_register(1 - it.bits(sym))
    assert len(m.events) == 1 and m.events[0].flags == it.INVERTED and list(m.events[0].sym[:len(sym)]) == sym


def _knock(bits, places, dots=20, nbits=1):
    """the bits with the first nbits of every place named turned over"""
    out = np.array(bits, np.uint8)
    for p in places:
        out[dots + 10 * p:dots + 10 * p + nbits] ^= 1
    return out


def test_either_copy_alone_gives_every_symbol():
    sym = it.individual_call(TO, FROM)
    n = len(sym)
    b = it.bits(sym)
    dx = _through_register(_knock(b, range(12, 12 + 2 * n, 2)))
    assert len(dx.events) == 1 and dx.events[0].from_rx == n and dx.events[0].flags == 0 and dx.events[0].holes == 0
    assert list(dx.events[0].sym[:n]) == sym
    rx = _through_register(_knock(b, range(17, 17 + 2 * n, 2)))
    assert len(rx.events) == 1 and rx.events[0].from_rx == 0 and rx.events[0].flags == 0 and list(rx.events[0].sym[:n]) == sym
    # a fade of 400 ms, four places in a row at a time, wherever it falls behind the phasing: nothing is lost
    for p0 in range(16, 2 * n + 12):
        m = _through_register(_knock(b, range(p0, p0 + 4)))
        e = m.events[0]
        assert len(m.events) == 1 and e.flags == 0 and e.holes == 0 and list(e.sym[:n]) == sym, p0
        assert e.from_rx == sum(1 for p in range(p0, p0 + 4) if p % 2 == 0 and p < 12 + 2 * n), p0


@pytest.mark.parametrize("i", [0, 1, 2, 9, 20, 22])
def test_one_hole_is_mended_on_the_host(i):
    """both copies of message symbol i gone (the error-check symbol itself at i = 22)"""
    sym = it.individual_call(TO, FROM)
    m = _through_register(_knock(it.bits(sym), (12 + 2 * i, 17 + 2 * i)))
    assert len(m.events) == 1
    e = m.events[0]
    assert (e.nsym, e.flags, e.holes, e.hole_mask, e.sym[i]) == (len(sym), it.CHECK, 1, 1 << i, it.HOLE)
    assert it.event_symbols(e) == sym[:i] + [None] + sym[i + 1:] and not it.parse(e)["ok"]
    r = it.repair(e)
    assert (r.flags, r.holes, r.hole_mask) == (0, 0, 0) and list(r.sym[:r.nsym]) == sym and r.sync_sample == e.sync_sample
    assert it.read(m.events)[0]["ok"] and it.read(m.events)[0]["to"] == "%09d" % TO
    # two holes are not mended, nor is a hole in the end of sequence ever filed by rule (a)
    two = _through_register(_knock(it.bits(sym), (12 + 2 * i, 17 + 2 * i, 12 + 2 * 5, 17 + 2 * 5))).events[0]
    assert two.holes == 2 and it.repair(two) is two


def test_a_wrong_symbol_fails_the_check():
    """both copies of symbol 4 carry another symbol: the code cannot see it, the check does"""
    sym = it.individual_call(TO, FROM)
    seq = it.sequence(sym)
    seq[12 + 2 * 4] = seq[17 + 2 * 4] = sym[4] ^ 3
    e = _through_register(it.place_bits(seq)).events[0]
    assert e.flags == it.CHECK and e.holes == 0 and e.sym[4] == sym[4] ^ 3 and it.repair(e) is e


@pytest.mark.parametrize("lose", [1, 3, 5])
def test_holes_in_a_row_end_the_message(lose):
    """rule (c): `lose` symbols unresolved in a row end the message; it is filed, marked lost, if eight were resolved
    before, and counted in aborted otherwise"""
    sym = it.individual_call(TO, FROM)
    b = it.bits(sym)
    for first, filed in ((10, True), (8, True), (7, False), (0, False)):
        gone = [p for i in range(first, first + lose) for p in (12 + 2 * i, 17 + 2 * i)]
        m = _through_register(_knock(b, gone)[:20 + 10 * (17 + 2 * (first + lose + 2))], lose=lose)
        assert (len(m.events), m.aborted, m.synced, m.nsym, m.nres, m.holes) == (int(filed), int(not filed), 0, first + lose, first, lose)
        if filed:
            e = m.events[0]
            assert (e.nsym, e.flags, e.holes, e.hole_mask) == (first + lose, it.LOST | it.CHECK, lose, ((1 << lose) - 1) << first)
            assert list(e.sym[:first]) == sym[:first] and set(e.sym[first:e.nsym]) == {it.HOLE} and not any(e.sym[e.nsym:])
            assert it.parse(e)["lost"] and not it.parse(e)["ok"] and it.repair(e) is e
    # one fewer in a row, and the message goes on to its end
    gone = [p for i in range(10, 10 + lose - 1) for p in (12 + 2 * i, 17 + 2 * i)]
    m = _through_register(_knock(b, gone), lose=lose)
    assert len(m.events) == 1 and m.events[0].nsym == len(sym) and m.events[0].holes == lose - 1 and m.run == 0


def test_sixty_four_symbols_without_an_end_are_filed_truncated():
    """rule (b); and a message of exactly 64 with its end in place is whole"""
    body = list(range(62))
    m = _through_register(it.bits(it.message(it.INDIVIDUAL, body[:60])))
    assert len(m.events) == 1 and m.events[0].flags == 0 and m.events[0].nsym == 64
    seq = [it.INDIVIDUAL] * 2 + body + [1, 2, 3, 4]             # no end of sequence among the first 64
    m = _through_register(it.bits(seq))
    assert len(m.events) == 1 and not m.synced
    e = m.events[0]
    assert (e.nsym, e.flags, e.holes) == (64, it.TRUNCATED | it.CHECK, 0) and list(e.sym) == seq[:64]
    assert it.parse(e)["truncated"] and not it.parse(e)["ok"]


def test_a_full_arena_counts_what_it_drops():
    b = np.concatenate([it.bits(it.individual_call(TO, FROM, frequency=()))] * 5)
    m = _through_register(b, max_events=3)
    assert len(m.events) == 3 and m.nevents == 5 and m.dropped == 2 and m.syncs == 5


def _calls(seed):
    rng = np.random.default_rng(seed)
    return it.individual_call(int(rng.integers(1, 10 ** 9)), int(rng.integers(1, 10 ** 9)))


@functools.lru_cache(maxsize=None)
def _read_under_noise(Fs, B, db):
    """of eight individual calls, each in a run of its own: filed whole with the check good; whole after the host's repair;
    and events that hold a symbol that was not sent"""
    good = mended = wrong = 0
    for seed in range(8):
        sym = _calls(seed)
        x = it.modulate(it.bits(sym), Fs, amp=AMP, lead=40, tail=10)
        x = x + np.random.default_rng(100 + seed).normal(0.0, dm.noise_sigma(AMP, db, Fs), len(x)).astype(np.float32)
        ev = dm.DscModel(Fs, B).feed(x).events
        good += any(e.flags == 0 and list(e.sym[:e.nsym]) == sym for e in ev)
        mended += any(r.flags == 0 and list(r.sym[:r.nsym]) == sym for r in map(it.repair, ev))
        wrong += sum(1 for e in ev if any(g is not None and (i >= len(sym) or g != sym[i]) for i, g in enumerate(it.event_symbols(e))))
    return good, mended, wrong


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
@pytest.mark.parametrize("db", [20, 14, 12])
def test_every_message_is_whole_from_20_to_12_db(Fs, B, db):
    good, mended, wrong = _read_under_noise(Fs, B, db)
    print("dsc noise", Fs, B, db, "dB:", good, "of 8 whole,", mended, "after repair,", wrong, "with a symbol that was not sent")
    assert good == 8 and wrong == 0


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
def test_loss_further_down_is_measured(Fs, B):
    """not asserted beyond the arithmetic: printed, and copied into the module's docstring, the header comment and DESIGN
    4.27"""
    for db in (10, 8, 6):
        good, mended, wrong = _read_under_noise(Fs, B, db)
        print("dsc noise", Fs, B, db, "dB:", good, "of 8 whole,", mended, "after repair,", wrong, "with a symbol that was not sent")
        assert 0 <= good <= mended <= 8


SECONDS = 240.0


@pytest.mark.parametrize("gate", [True, False])
def test_noise_alone_files_nothing(gate):
    """white noise at amplitude 0.1: with the gate, and by the phasing sequence and the symbol code alone"""
    Fs, B = 12000.0, 12
    rng = np.random.default_rng(6)
    m = dm.DscModel(Fs, B, gate=gate)
    ratio = []
    for at in range(int(SECONDS)):
        m.feed(rng.normal(0.0, 0.1, int(Fs)).astype(np.float32))
        if at >= 2:
            ratio.append(16.0 * m.sig / m.nse)
    print("dsc noise alone, %g s, gate %s: 16 sig / nse from %.1f to %.1f, mean %.1f; bits open %d of %d; syncs %d, aborted %d"
          % (SECONDS, gate, min(ratio), max(ratio), np.mean(ratio), sum(v for _, v in m.bits), len(m.bits), m.syncs, m.aborted))
    assert not m.events and m.nevents == 0
    assert gate or all(v for _, v in m.bits)


@pytest.mark.parametrize("gate", [True, False])
def test_a_steady_tone_on_mark_files_nothing(gate):
    """the gate is wide open on it either way; ten equal bits are no symbol"""
    Fs, B = 12000.0, 12
    x = it.modulate(np.ones(int(SECONDS * 100), np.uint8), Fs, amp=AMP, lead=0, tail=0)
    m = dm.DscModel(Fs, B, gate=gate).feed(x)
    print("dsc steady tone, %g s, gate %s: bits open %d of %d" % (SECONDS, gate, sum(v for _, v in m.bits), len(m.bits)))
    assert sum(v for _, v in m.bits) > len(m.bits) - 100 and {b for b, _ in m.bits[10:]} == {1}
    assert not m.events and m.nevents == 0 and m.syncs == 0


def test_the_clock_holds_through_equal_bits_and_settles_on_the_dots():
    """200 dots, then 300 equal bits (30 places of a steady tone), then the sequence: the clock that the dots set is still
    right when the phasing comes, and the sampling point lies within an eighth of a bit of the middle"""
    Fs, B = 12000.0, 12
    sym = it.individual_call(TO, FROM, frequency=())
    b = np.concatenate([it.bits(sym, 200)[:200], np.ones(300, np.uint8), it.bits(sym)])
    x = it.modulate(b, Fs, amp=AMP, lead=0, tail=8)
    m = dm.DscModel(Fs, B).feed(x)
    assert len(m.events) == 1 and m.events[0].flags == 0 and m.events[0].from_rx == 0
    got = "".join(str(v) for v, _ in m.bits)
    at = got.find("".join(map(str, b[150:520])))
    assert at >= 0, "the bits from the dots through the tone into the sequence come out in one piece"
    # centred, the window of a bit's centre point ends with the bit, and the late point lies a quarter bit behind it
    late = m.events[0].end_sample / B - (len(b) * m.tb / 256.0 + m.q / 256.0)
    print("dsc clock: the last late point ends %.2f frames behind where a centred clock puts it" % late)
    assert -1.0 <= late <= 3.0, "a frame's grain, and a fifth of a bit"


def test_every_starting_phase_is_read():
    """a short call behind noise at 48 starting phases of the clock against the bits, with white noise at 20 dB and a dot
    pattern of 20 bits.  Half a bit out, early and late read alike and the three-point walk has no slope; step 1's push
    carries the clock away from there.  Without it (the model only) the count that stays there is printed"""
    Fs, B = 12000.0, 12
    sym = it.individual_call(TO, FROM, frequency=())
    lost = {True: 0, False: 0}
    for nudge in lost:
        for trial in range(48):
            x = it.modulate(it.bits(sym), Fs, amp=AMP, lead=30 + trial / 16.0, tail=6)
            x = x + np.random.default_rng(trial * 3).normal(0.0, dm.noise_sigma(AMP, 20.0, Fs), len(x)).astype(np.float32)
            ev = dm.DscModel(Fs, B, nudge=nudge).feed(x).events
            lost[nudge] += not (len(ev) == 1 and ev[0].flags == 0 and list(ev[0].sym[:len(sym)]) == sym)
    print("dsc starting phases: messages lost of 48 with the push", lost[True], "and without", lost[False])
    assert lost[True] == 0


def test_widest_intermediates_stay_inside_the_header_bounds():
    """a full-scale square wave at B = 256, W = 32: kq_rtty_*'s bounds on the frame sums, the reduced sums, the window sums
    and the powers"""
    Fs, B = 1024000.0, 256
    n = np.arange(40 * 8192)
    x = np.sign(np.cos(2 * np.pi * 1250.0 / Fs * n)).astype(np.float32)
    m = dm.DscModel(Fs, B, mark=1250.0, space=1500.0, baud=125.0).feed(x)
    assert m.W == 32
    wd = m.widest
    print("dsc widest", {k: v.bit_length() for k, v in wd.items()})
    assert wd["acc"] < 1 << 38 and wd["red"] < 1 << 26 and wd["sum"] < 1 << 31 and wd["P"] < 1 << 63 and wd["P"] > 1 << 58
