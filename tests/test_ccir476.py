"""The CCIR 476 alphabet and the NAVTEX format helpers (ka9q_sdr_amd/ccir476.py) on the CPU.  The table is written down
from memory; what can be held against something else is held here: it uses each of the C(7,4) = 35 words with four B exactly
once, and for the 25 ITA2 combinations with two, three or four marks its words carry the ITA2 code of baudot.LETTERS, a
table of another origin, in bits 2..6.  Which of the ten words left over is which has no such check.  Then the shifts, the
DX / RX interleave and the cut of a text into ZCZC .. NNNN messages."""
import collections
import itertools

import pytest

from ka9q_sdr_amd import baudot, ccir476 as cc

Ev = collections.namedtuple("Ev", "code flags")


def test_the_table_uses_every_constant_ratio_word_once():
    words = [w for w in range(128) if bin(w).count("1") == 4]
    assert len(words) == 35 and len(cc.CODE) == 35
    assert sorted(cc.CODE.values()) == words and all(cc.is_character(c) for c in cc.CODE.values())
    assert all(len(w) == 7 and set(w) <= {"B", "Y"} and w.count("B") == 4 for w in cc.WORDS.values())
    assert (cc.ALPHA, cc.BETA, cc.REP) == (0x78, 0x66, 0x33) and cc.CODE["A"] == 0x71 and cc.CODE["SPACE"] == 0x1D
    for w in cc.CODE.values():                                   # any single wrong bit is seen
        assert not any(cc.is_character(w ^ 1 << b) for b in range(7))
    assert not cc.is_character(0) and not cc.is_character(127)   # a steady tone is no character


def test_the_ita2_code_sits_in_bits_2_to_6():
    """every ITA2 combination with two, three or four marks: the 24 letters other than E and T, and FIGS"""
    held = []
    for k, ch in enumerate(baudot.LETTERS):
        if not 2 <= bin(k).count("1") <= 4:
            continue
        name = "FIGS" if k == baudot.FIGS else ch
        assert name in cc.WORDS, (k, ch)
        sent = "".join("B" if k >> i & 1 else "Y" for i in range(5))          # ITA2 sends its lowest bit first
        assert cc.WORDS[name][1:6] == sent, (name, cc.WORDS[name], sent)
        held.append(name)
    assert len(held) == 25 and "FIGS" in held and "E" not in held and "T" not in held
    assert sorted(n for n in held if n != "FIGS") == sorted(set("ABCDEFGHIJKLMNOPQRSTUVWXYZ") - set("ET"))
    assert cc.WORDS["A"] == "B" + "BBYYY" + "B" and cc.WORDS["R"] == "B" + "YBYBY" + "B"
    rest = sorted(set(cc.WORDS) - set(held))
    assert rest == sorted(["E", "T", "SPACE", "CR", "LF", "LTRS", "BLANK", "ALPHA", "BETA", "REP"])   # from memory alone


def _events(codes):
    return [Ev(c, 0) for c in codes]


def test_text_round_trips_through_the_shifts():
    for text in ("CQ DE NAVTEX", "ZCZC FA01\r\nGALE WARNING 7/8 NW-LY 1005 HPA.\r\nNNNN", "A1B2C3", "12 34", "(=+:?)", ""):
        codes = cc.codes_of(text)
        assert codes[0] == cc.LTRS and all(cc.is_character(c) for c in codes)
        assert cc.read_text(_events(codes)) == text, text
    assert cc.codes_of("A1") == [cc.LTRS, cc.CODE["A"], cc.FIGS, cc.CODE["Q"]]
    assert cc.codes_of("1A") == [cc.LTRS, cc.FIGS, cc.CODE["Q"], cc.LTRS, cc.CODE["A"]]
    assert cc.codes_of("a b") == cc.codes_of("A B") and cc.codes_of("1 2").count(cc.FIGS) == 1   # a space keeps the case
    with pytest.raises(ValueError):
        cc.codes_of("A$")


def test_a_figure_on_every_key():
    keys = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    assert sorted(cc.FIGURES) == list(keys)
    assert "".join(cc.FIGURES[k] for k in keys) == "-?:\x053\0\0\08\a().,9014'57=2/6+"
    printed = [f for f in cc.FIGURES.values() if f != "\0"]
    assert len(printed) == 23 and len(set(printed)) == 23
    for k in keys:
        f = cc.FIGURES[k]
        got = cc.read_text(_events([cc.FIGS, cc.CODE[k], cc.LTRS, cc.CODE[k]]))
        assert got == (f if f != "\0" else "") + k, k
        if f != "\0":
            assert cc.codes_of(f) == [cc.LTRS, cc.FIGS, cc.CODE[k]], k
    # unresolved characters print *, in either case; beta, BLANK and stray service signals print nothing
    ev = [Ev(cc.CODE["A"], 0), Ev(cc.NONE, cc.UNRESOLVED), Ev(cc.BETA, 0), Ev(cc.BLANK, 0), Ev(cc.ALPHA, cc.DIFFER), Ev(cc.REP, 0),
          Ev(cc.CODE["B"], cc.FROM_RX | cc.INVERTED)]
    assert cc.read_text(ev) == "A*B"


def test_the_interleave():
    codes = cc.codes_of("NAVTEX 518")
    n = len(codes)
    p = cc.places(codes, phasing=(0, 0))
    assert len(p) == 2 * n + 6
    for i, c in enumerate(codes):
        assert p[2 * i] == c and p[2 * i + 5] == c, i
    used = {2 * i for i in range(n)} | {2 * i + 5 for i in range(n)}
    for k, w in enumerate(p):
        if k not in used:
            assert w == (cc.ALPHA if k & 1 else cc.REP), k
    assert p[1] == p[3] == cc.ALPHA and p[2 * n] == p[2 * n + 2] == p[2 * n + 4] == cc.REP
    q = cc.places(codes, phasing=(7, 3))
    assert q[:14] == [cc.REP, cc.ALPHA] * 7 and q[14:14 + len(p)] == p and q[14 + len(p):] == [cc.REP, cc.ALPHA] * 3
    b = cc.bits(q)
    assert len(b) == 7 * len(q) and "".join(map(str, b[:14])) == "01100111111000"
    assert "".join("BY"[1 - v] for v in b[14 * 7 + 7 * 2:14 * 7 + 7 * 3]) == cc.WORDS[cc.NAME[codes[1]]]
    with pytest.raises(ValueError):
        cc.places([0x7F])
    assert cc.navtex_config(12000.0) == dict(block_len=12) and cc.navtex_config(48000.0) == dict(block_len=48)


def test_phasing_has_one_alignment():
    """the header's argument for step 4: in a stream of phasing signals, at any alignment that is off by other than a
    multiple of seven bits, at most two of the last four places read as the phasing signals they would have to be"""
    stream = cc.bits([cc.REP, cc.ALPHA] * 6).tolist()
    for off in range(14):
        x = int("".join(map(str, stream[off:off + 28])), 2)
        c = [x >> (7 * i) & 127 for i in range(4)]
        as_rx = sum(c[i] == (cc.ALPHA, cc.REP)[i & 1] for i in range(4))
        as_dx = sum(c[i] == (cc.REP, cc.ALPHA)[i & 1] for i in range(4))
        assert (as_rx, as_dx) == ((4, 0) if off == 0 else (0, 4) if off == 7 else (as_rx, as_dx)) and (off % 7 == 0 or max(as_rx, as_dx) <= 2)


BODY = "GALE WARNING\r\nFORTIES NW 7/8"
ONE = "ZCZC FA01\r\n" + BODY + "\r\nNNNN"


def test_messages():
    assert cc.messages(ONE) == [cc.Message("F", "A", "01", BODY, True)]
    assert cc.messages("\r\n\r\n" + ONE + "\r\n\r\n") == [cc.Message("F", "A", "01", BODY, True)]
    cut_end = ONE[:-12]                                          # the end not seen
    assert cc.messages(cut_end) == [cc.Message("F", "A", "01", ONE[11:-12].strip("\r\n "), False)]
    cut_start = ONE[20:]                                         # joined late: no header
    assert cc.messages(cut_start) == [cc.Message(None, None, None, ONE[20:-4].strip("\r\n "), True)]
    two = ONE + "\r\n\r\nZCZC GB17\r\nNIL\r\nNNNN\r\n"
    assert cc.messages(two) == [cc.Message("F", "A", "01", BODY, True), cc.Message("G", "B", "17", "NIL", True)]
    assert cc.messages(cut_start + "\r\n" + two)[0].station is None and len(cc.messages(cut_start + "\r\n" + two)) == 3
    assert cc.messages("") == [] and cc.messages("NOTHING HERE") == []
    # a message whose NNNN was lost runs into the next header and is cut there
    lost = ONE[:-4] + "ZCZC GB17\r\nNIL\r\nNNNN"
    assert [m.complete for m in cc.messages(lost)] == [False, True] and cc.messages(lost)[1].serial == "17"
    assert cc.read_text(_events(cc.codes_of(ONE))) == ONE
