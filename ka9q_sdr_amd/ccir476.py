"""NAVTEX / SITOR-B (CCIR 476, ITU-R M.476 and M.625, collective B mode) beside the NAVTEX decoder bank (navtex.py,
include/ka9q_hip.h: kq_navtex_*), plain Python and numpy, no device: the seven-bit alphabet with its letters and figures
case, a text as code words with the shifts put in, the DX / RX interleave with its phasing signals, the bits and
phase-continuous 2-FSK for test traffic, the bank's geometry for a sample rate, the reader of the bank's events, and the
cut of a text into ZCZC .. NNNN messages.

Written down from memory: no copy of the Recommendations was at hand.  Two things about the table are held by
tests/test_ccir476.py: it uses each of the C(7,4) = 35 words with four B exactly once; and for the 25 ITA2 combinations with
two, three or four marks (the 24 letters other than E and T, and FIGS) bits 2..6 of the word, in sending order, are the
ITA2 code in sending order, against baudot.LETTERS, a table of another origin.  FROM MEMORY ALONE, with no such check:
which of the ten words left over is which of E, T, SPACE, CR, LF, LTRS, BLANK, alpha, beta and rep; the figures case
(international ITA2, not baudot.py's US-TTY); that character i goes out in DX place 2 i and RX place 2 i + 5, with rep in
the DX and alpha in the RX places while phasing; which audio tone is state B on which sideband (MARK and SPACE below are
kq_dsc_*'s guess, which the decoder does not depend on: it takes the complement as well).  Nothing here has met a signal
off the air.
"""
import collections

import numpy as np

from . import itu493

BAUD, MARK, SPACE = 100.0, 1785.0, 1615.0                            # a USB channel 1700 Hz below the assigned frequency
UNRESOLVED, FROM_RX, DIFFER, INVERTED = 1, 2, 4, 8                   # an event's flag bits
NONE = 0x7F                                                          # an event's code where neither copy gave a character

# B = mark = 1, in sending order, the first bit on the left
WORDS = dict(A="BBBYYYB", B="YBYYBBB", C="BYBBBYY", D="BBYYBYB", E="YBBYBYB", F="BBYBBYY", G="BYBYBBY", H="BYYBYBB", I="BYBBYYB",
             J="BBBYBYY", K="YBBBBYY", L="BYBYYBB", M="BYYBBBY", N="BYYBBYB", O="BYYYBBB", P="BYBBYBY", Q="YBBBYBY", R="BYBYBYB",
             S="BBYBYYB", T="YYBYBBB", U="YBBBYYB", V="YYBBBBY", W="BBBYYBY", X="YBYBBBY", Y="BBYBYBY", Z="BBYYYBB",
             CR="YYYBBBB", LF="YYBBYBB", LTRS="YBYBBYB", FIGS="YBBYBBY", SPACE="YYBBBYB", BLANK="YBYBYBB", ALPHA="BBBBYYY",
             BETA="BBYYBBY", REP="YBBYYBB")
CODE = {name: int(w.replace("B", "1").replace("Y", "0"), 2) for name, w in WORDS.items()}   # the first bit sent in bit 6
NAME = {c: name for name, c in CODE.items()}
ALPHA, BETA, REP = CODE["ALPHA"], CODE["BETA"], CODE["REP"]          # phasing 1 (RX), idle, phasing 2 (DX)
LTRS, FIGS, BLANK = CODE["LTRS"], CODE["FIGS"], CODE["BLANK"]
WRU, BELL = "\x05", "\a"
# the figures case by the letter that shares the key; F, G and H are unassigned (\0: nothing is printed)
FIGURES = dict(A="-", B="?", C=":", D=WRU, E="3", F="\0", G="\0", H="\0", I="8", J=BELL, K="(", L=")", M=".", N=",", O="9", P="0",
               Q="1", R="4", S="'", T="5", U="7", V="=", W="2", X="/", Y="6", Z="+")
BOTH = {"\r": CODE["CR"], "\n": CODE["LF"], " ": CODE["SPACE"]}      # the same in either case
_LTR = {k: CODE[k] for k in FIGURES}
_FIG = {f: CODE[k] for k, f in FIGURES.items() if f != "\0"}
_PRINT_L = {**{CODE[k]: k for k in FIGURES}, **{c: ch for ch, c in BOTH.items()}}
_PRINT_F = {**{CODE[k]: f for k, f in FIGURES.items()}, **{c: ch for ch, c in BOTH.items()}}

Message = collections.namedtuple("Message", "station subject serial body complete")


def is_character(w):
    """a seven-bit word with exactly four B"""
    return 0 <= int(w) < 128 and bin(int(w)).count("1") == 4


def codes_of(text):
    """the code words of a text (letters in either case, the figures above, CR, LF and space), with FIGS and LTRS where
    the case changes; the sender starts in the letters case and says so with LTRS"""
    out, figs = [LTRS], False
    for ch in text:
        ch = ch.upper()
        if ch in BOTH:
            out.append(BOTH[ch])
        elif ch in _LTR:
            if figs:
                out.append(LTRS)
                figs = False
            out.append(_LTR[ch])
        elif ch in _FIG:
            if not figs:
                out.append(FIGS)
                figs = True
            out.append(_FIG[ch])
        else:
            raise ValueError("no code word for %r" % ch)
    return out


def places(codes, phasing=(20, 4)):
    """the word of every place: phasing[0] pairs of (rep, alpha) ahead; then, counting from there, character i in DX place
    2 i and in RX place 2 i + 5, with rep and alpha in the places a copy has not reached yet or has already left; then
    phasing[1] pairs behind.  2 (phasing[0] + len(codes) + 3 + phasing[1]) places"""
    ahead, behind = phasing
    codes = [int(c) for c in codes]
    if any(not is_character(c) for c in codes):
        raise ValueError("a code word has four B of seven")
    n = len(codes)
    out = [REP, ALPHA] * ahead
    for p in range(2 * n + 6):
        if p & 1:
            i = (p - 5) >> 1
            out.append(codes[i] if 0 <= i < n else ALPHA)
        else:
            out.append(codes[p >> 1] if (p >> 1) < n else REP)
    return out + [REP, ALPHA] * behind


def bits(place_words):
    """the seven bits of every place, the first sent first, uint8"""
    return np.array([w >> s & 1 for w in place_words for s in range(6, -1, -1)], np.uint8)


def modulate(bit_values, fs, baud=BAUD, mark=MARK, space=SPACE, amp=0.3, lead=8, ppm=0.0, tail=4):
    """phase-continuous FSK, float32: itu493.modulate with NAVTEX's tones (state B at `mark`, Y at `space`)"""
    return itu493.modulate(bit_values, fs, baud, mark, space, amp, lead, ppm, tail)


def navtex_config(fs, baud=BAUD):
    """NavtexBank keywords for a sample rate: the frame (8 to 256 samples) nearest to ten in a bit, with 8 to 32 in it"""
    return itu493.dsc_config(fs, baud)


def read_text(events):
    """the events of one slot (anything with `code` and `flags`) as text, through the shift state, which starts at
    letters: `*` for an unresolved character; beta, BLANK and a stray alpha or rep print nothing, nor do the shifts
    themselves and the unassigned figures"""
    out, figs = [], False
    for e in events:
        code = int(e.code)
        if int(e.flags) & UNRESOLVED or code not in NAME:
            out.append("*")
        elif code == LTRS:
            figs = False
        elif code == FIGS:
            figs = True
        elif code in _PRINT_L:
            ch = (_PRINT_F if figs else _PRINT_L)[code]
            if ch != "\0":
                out.append(ch)
    return "".join(out)


def messages(text):
    """the NAVTEX messages of a text, in order, each a Message: station (B1), subject (B2), serial (B3 B4), body (what
    lies between the header line and NNNN, without the line ends around it) and complete (NNNN was seen).  What stands
    ahead of the first ZCZC is a message cut at its start if it ends with NNNN: station, subject and serial are None"""
    out = []
    at = text.find("ZCZC")
    head = text[:at] if at >= 0 else text
    if "NNNN" in head:
        out.append(Message(None, None, None, head[:head.index("NNNN")].strip("\r\n "), True))
    while at >= 0:
        nxt = text.find("ZCZC", at + 4)
        part = text[at + 4:nxt if nxt >= 0 else len(text)]
        end = part.find("NNNN")
        complete = end >= 0
        if complete:
            part = part[:end]
        ident = part.lstrip(" ")[:4]
        body = part.lstrip(" ")[4:].strip("\r\n ")
        if len(ident) == 4:
            out.append(Message(ident[0], ident[1], ident[2:4], body, complete))
        else:
            out.append(Message(None, None, None, "", complete))
        at = nxt
    return out


__all__ = ["BAUD", "MARK", "SPACE", "UNRESOLVED", "FROM_RX", "DIFFER", "INVERTED", "NONE", "WORDS", "CODE", "NAME", "ALPHA", "BETA",
           "REP", "LTRS", "FIGS", "BLANK", "WRU", "BELL", "FIGURES", "BOTH", "Message", "is_character", "codes_of", "places", "bits",
           "modulate", "navtex_config", "read_text", "messages"]
