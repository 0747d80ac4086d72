"""ka9q_sdr_amd/eas.py on the CPU, with no decoder in the way: the header's text and its parse, the field limits, the bit
order of a burst, the reader of events, the vote over three bursts and over two, and the test audio's bit edges.  The format
is written down from memory (eas.py says so): these tests hold the module consistent with itself and with the issue's
description of the signal, not with the rule's text."""
import collections

import numpy as np
import pytest

from ka9q_sdr_amd import eas

Ev = collections.namedtuple("Ev", "code flags index errs end_sample")


def _events(text, start, bad=(), reason=eas.COMPLETE, step=100):
    """the events of one header burst as the bank files them: START, a byte each behind ZCZC, END"""
    out = [Ev(ord("Z"), eas.START, 0, 0, start)]
    for k, b in enumerate(text.encode("latin-1")[4:]):
        out.append(Ev(b, eas.BAD if k + 4 in bad else 0, k, 0, start + step * (k + 1)))
    return out + [Ev(reason, eas.END, len(text) - 4, 0, out[-1].end_sample)]


def test_header_and_parse_round_trip():
    text = eas.header("WXR", "TOR", ["039173", 39035], (0, 30), (159, 20, 15), "KCLE-NWS")
    assert text == "ZCZC-WXR-TOR-039173-039035+0030-1592015-KCLE/NWS-"
    h = eas.parse(text)
    assert h == eas.Header("WXR", "TOR", "Tornado Warning", ["039173", "039035"], 30, (159, 20, 15), "KCLE/NWS")
    assert eas.parse(eas.header("CIV", "XYZ", [1], "1245", "3662359", "AB")) == \
        eas.Header("CIV", "XYZ", "XYZ", ["000001"], 12 * 60 + 45, (366, 23, 59), "AB")       # an unknown event passes through
    assert set(eas.ORIGINATORS) == {"EAS", "CIV", "WXR", "PEP"}
    assert all(k in eas.EVENTS for k in ("RWT", "RMT", "TOR", "SVR", "EAN", "NPT")) and all(len(k) == 3 for k in eas.EVENTS)


@pytest.mark.parametrize("text", [
    "", "NNNN", "ZCZC-WXR-TOR+0030-1592015-KCLE/NWS-",                       # no location
    "ZCZC-ABC-TOR-039173+0030-1592015-KCLE/NWS-",                             # no such originator
    "ZCZC-WXR-TOR-039173+0030-1592015-KCLE/NWS",                              # the last dash
    "ZCZC-WXR-TOR-039173+0030-1592015-KCLE/NWS-X",                            # something behind it
    "ZCZC-WXR-TOR-39173+0030-1592015-KCLE/NWS-",                              # five digits
    "ZCZC-WXR-TOR-039173*0030-1592015-KCLE/NWS-",                             # the plus
    "ZCZC-WXR-TOR-039173+0030-1592415-KCLE/NWS-",                             # 24 h
    "ZCZC-WXR-TOR-039173+0030-0002015-KCLE/NWS-",                             # day 0
    "ZCZC-WXR-TOR-039173+0030-1592015-KCLE/NW-",                              # a station of seven
    "ZCZC-WXR-TOR" + "-039173" * 32 + "+0030-1592015-KCLE/NWS-"])             # 32 locations
def test_parse_refuses_what_is_outside_the_grammar(text):
    with pytest.raises(ValueError):
        eas.parse(text)


def test_field_limits():
    locs = ["%06d" % k for k in range(31)]
    text = eas.header("EAS", "RWT", locs, "0100", "0011234", "WXYZ/FM")
    assert len(text) == 252 == eas.MAX_BYTES and eas.parse(text).locations == locs and eas.parse(text).station == "WXYZ/FM"
    for bad in ([], locs + ["000031"]):
        with pytest.raises(ValueError, match="1 to 31 location codes"):
            eas.header("EAS", "RWT", bad, "0100", "0011234", "WXYZ/FM")
    with pytest.raises(ValueError, match="eight characters"):
        eas.header("EAS", "RWT", locs, "0100", "0011234", "WXYZ/FM/1")
    with pytest.raises(ValueError):
        eas.header("EAS", "RWT", ["12345"], "0100", "0011234", "WXYZ/FM")


def test_bit_order_of_a_burst():
    b = eas.burst("ZCZC")
    assert b.dtype == np.uint8 and len(b) == 8 * (16 + 4)
    assert b[:8].tolist() == [1, 1, 0, 1, 0, 1, 0, 1]                         # 0xAB, the least significant bit first
    assert all(b[8 * k:8 * k + 8].tolist() == b[:8].tolist() for k in range(16))
    assert b[128:136].tolist() == [0, 1, 0, 1, 1, 0, 1, 0] and b[136:144].tolist() == [1, 1, 0, 0, 0, 0, 1, 0]    # 'Z' 0x5A, 'C' 0x43
    assert not b[135::8].any()                                                # bit 7 is always 0


def test_read_cuts_the_events_into_bursts():
    text = eas.header("WXR", "RWT", [12345], "0015", "1231200", "KABC/FM")
    cut = text[:7] + "\xc1" + text[8:20]                                     # a byte outside 0x20..0x7E, flagged BAD
    ev = _events(text, 1000) + [Ev(ord("N"), eas.START, 0, 1, 90000)] + _events(cut, 100000, bad=(7,), reason=eas.LOST)
    ev += [Ev(ord("Z"), eas.START, 0, 2, 200000), Ev(ord("-"), 0, 0, 0, 200100)]              # still open at the end
    got = eas.read(ev)
    assert [b.kind for b in got] == ["Z", "N", "Z", "Z"]
    assert got[0] == eas.Burst("Z", text, text.encode(), [], eas.COMPLETE, 0, 1000, 1000 + 100 * (len(text) - 4))
    assert got[1] == eas.Burst("N", "NNNN", b"NNNN", [], 0, 1, 90000, 90000)
    assert got[2].text == text[:7] + "?" + text[8:20] and got[2].bad == [7] and got[2].reason == eas.LOST
    assert got[2].data == cut.encode("latin-1")                                  # the byte as read stays in data
    assert got[3] == eas.Burst("Z", "ZCZC-", b"ZCZC-", [], 0, 2, 200000, 200100)
    assert eas.read([]) == [] and eas.read(ev[3:6]) == []                      # bytes with no START ahead of them


def _burst(text, start, flips=()):
    data = bytearray(text.encode())
    for at, bit in flips:
        data[at] ^= 1 << bit
    return eas.read(_events(data.decode("latin-1"), start, bad=[k for k, v in enumerate(data) if not 0x20 <= v <= 0x7E]))[0]


def test_vote_on_three_bursts_with_disjoint_errors():
    fs = 48000.0
    text = eas.header("WXR", "SVR", [39173, 39035, 39093], "0045", "1592015", "KCLE/NWS")
    three = [_burst(text, 0, [(5, 0), (30, 7)]), _burst(text, 100000, [(12, 3)]), _burst(text, 200000, [(6, 1), (40, 2), (41, 6)])]
    assert all(b.text != text for b in three) and three[0].bad == [30]
    assert eas.vote(three, fs) == [eas.Alert(text, 3, 0)]
    # two bursts wrong in the same bit are outvoted: the vote is no checksum
    same = [_burst(text, 0, [(12, 3)]), _burst(text, 100000, [(12, 3)]), _burst(text, 200000)]
    assert eas.vote(same, fs)[0].text == three[1].text
    # a burst that ran on past the grammar's end (its + was read wrong) and a short one do not shift the others
    ran_on = _burst(text.replace("+", "*") + "garbage!", 100000)
    short = eas.read(_events(text[:40], 200000, reason=eas.LOST))[0]
    assert eas.vote([three[1], ran_on, _burst(text, 200000)], fs)[0].text == text
    assert eas.vote([_burst(text, 0), ran_on, short], fs)[0].text == text
    # two alerts a minute apart are voted apart; ends of message take no part
    later = [b._replace(start_sample=b.start_sample + 60 * 48000) for b in three]
    eom = eas.Burst("N", "NNNN", b"NNNN", [], 0, 0, 500000, 500000)
    assert eas.vote(three + [eom] + later, fs) == [eas.Alert(text, 3, 0), eas.Alert(text, 3, 60 * 48000)]


def test_vote_on_two_bursts():
    fs = 48000.0
    text = eas.header("PEP", "EAN", [0], "0100", "0010000", "WHITEHSE")
    a, b = _burst(text, 0), _burst(text, 100000)
    assert eas.vote([a, b], fs) == [eas.Alert(text, 2, 0)]
    assert eas.vote([a, _burst(text, 100000, [(9, 1)])], fs) == []             # two that differ decide nothing
    assert eas.vote([a], fs) == [] and eas.vote([], fs) == []
    assert eas.vote([a, b._replace(start_sample=20 * 48000)], fs) == []        # too far apart to be one alert's


def test_clip():
    text = eas.header("WXR", "RWT", [12345], "0015", "1231200", "KABC/FM")
    assert eas.clip(text) == text and eas.clip(text + "xyz-") == text and eas.clip(text[:-1]) == text[:-1]
    assert eas.clip("ZCZC-no plus") == "ZCZC-no plus"


def test_afsk_turns_the_tone_over_at_the_exact_edge():
    """a bit is 92.16 samples at 48 kHz: the phase is continuous, and between two samples that an edge separates it advances
    by the two frequencies' shares of the step"""
    fs = 48000.0
    per = fs / eas.BAUD
    assert abs(per - 92.16) < 1e-9
    bits = np.array([1, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    n0, x = eas.afsk(bits, fs, start=10.25, amp=1.0)
    assert n0 == 11 and len(x) == int(np.ceil(10.25 + 8 * per)) - 11
    f = np.where(bits != 0, eas.MARK, eas.SPACE)
    for k in range(len(x)):
        t = n0 + k - 10.25
        i = min(int(t / per), 7)
        cycles = (f[:i].sum() * per + f[i] * (t - i * per)) / fs
        assert abs(x[k] - np.cos(2 * np.pi * cycles)) < 1e-9
    # four cycles of mark and three of space to a bit
    assert abs(eas.MARK * per / fs - 4.0) < 1e-12 and abs(eas.SPACE * per / fs - 3.0) < 1e-12


def test_modulate_lays_the_bursts_a_second_apart():
    fs = 48000.0
    text = eas.header("WXR", "RWT", [12345], "0015", "1231200", "KABC/FM")
    n = 8 * (16 + len(text)) * fs / eas.BAUD
    x = eas.modulate(text, fs, eom=False, lead=0.5, tail=0.5, amp=0.25)
    assert x.dtype == np.float32 and abs(len(x) - (fs + 3 * n + 2 * fs)) <= 2 and np.abs(x).max() <= 0.25
    on = np.abs(x) > 0
    edges = np.flatnonzero(np.diff(on.astype(np.int8)) != 0)
    quiet = [(b - a) for a, b in zip(edges[1::2], edges[2::2])]
    assert len(edges) >= 6 and max(abs(q - fs) for q in sorted(quiet)[-2:]) <= 2       # (a sample at a zero crossing aside)
    whole = eas.modulate(text, fs, attention="broadcast", attention_seconds=2.0, lead=0.5, tail=0.5)
    ne = 8 * (16 + 4) * fs / eas.BAUD
    assert abs(len(whole) - (fs + 3 * n + 3 * fs + 2 * fs + fs + 3 * ne + 2 * fs)) <= 4
    fast = eas.modulate(text, fs, eom=False, lead=0.5, tail=0.5, ppm=5000.0)
    assert abs(len(fast) - len(x) / 1.005) <= 3
    assert eas.same_config(48000.0) == dict(block_len=9) and eas.same_config(39062.5) == dict(block_len=8)
    with pytest.raises(ValueError):
        eas.same_config(12000.0)
