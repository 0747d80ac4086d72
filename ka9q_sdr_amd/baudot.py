"""The teleprinter alphabet beside the RTTY decoder bank (rtty.py, include/ka9q_hip.h: kq_rtty_*), plain Python: ITA2 with
the US-TTY figures case as data, the bank's geometry for a baud rate, continuous-phase FSK for test traffic and the reader
of the bank's events.

A character's code is its data bits, the first sent in the lowest place (E, sent mark space space space space, is 1).
The bank hands out raw codes; the shift state (letters / figures) is kept here.
"""
import numpy as np

NUL, LF, SPACE, CR, FIGS, LTRS = 0, 2, 4, 8, 27, 31
BELL = "\a"
LETTERS = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG\x0eMXV\x0f"              # by code; \x0e and \x0f stand where FIGS and LTRS are
FIGURES = "\x003\n- " + BELL + "87\r$4',!:(5\")2#6019?&\x0e./;\x0f"   # US-TTY
assert len(LETTERS) == 32 and len(FIGURES) == 32
BOTH = {NUL, LF, SPACE, CR, FIGS, LTRS}                              # the same in either case
_LTR = {c: k for k, c in enumerate(LETTERS) if k not in (FIGS, LTRS)}
_FIG = {c: k for k, c in enumerate(FIGURES) if k not in (FIGS, LTRS)}

FRAMING_ERROR = 1                                                    # an event's flag bit 0


def codes_of(text, unshift_on_space=True):
    """the ITA2 codes of a text, with FIGS and LTRS where the case changes; the sender starts with LTRS, and (as the reader
    does by default) falls back to letters on a space"""
    out, figs = [LTRS], False
    for ch in text.upper():
        if ch in _LTR and _LTR[ch] in BOTH:
            out.append(_LTR[ch])
            if ch == " " and unshift_on_space:
                figs = False
            continue
        if ch in _LTR:
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
            raise ValueError("no ITA2 code for %r" % ch)
    return out


def read_text(events, unshift_on_space=True, keep_framing_errors=False):
    """the events of one slot (anything with `code` and `flags`) as text: the low five bits of every code through the
    shift state, which starts at letters.  Characters filed with a framing error are left out unless asked for; NUL
    prints nothing."""
    out, figs = [], False
    for e in events:
        if (int(e.flags) & FRAMING_ERROR) and not keep_framing_errors:
            continue
        c = int(e.code) & 31
        if c == FIGS:
            figs = True
        elif c == LTRS:
            figs = False
        elif c != NUL:
            out.append((FIGURES if figs else LETTERS)[c])
            if c == SPACE and unshift_on_space:
                figs = False
    return "".join(out)


def rtty_config(fs, baud):
    """RttyBank keywords for a baud rate: the longest frame (8 to 256 samples) that leaves ten frames in a bit"""
    block_len = int(float(fs) / (10.0 * float(baud)) + 1e-9)
    if block_len < 8:
        raise ValueError("%g Hz is too slow for %g baud" % (fs, baud))
    return dict(block_len=min(block_len, 256))


def keying(codes, nbits=5, stop=1.5):
    """the characters as (mark?, bits) pairs: a start bit of space, the data bits from the lowest up, `stop` bits of mark"""
    out = []
    for c in codes:
        out.append((False, 1.0))
        out += [(bool(int(c) >> i & 1), 1.0) for i in range(nbits)]
        out.append((True, float(stop)))
    return out


def encode(text, baud, fs, mark=2125.0, space=2295.0, amp=0.3, nbits=5, stop=1.5, lead=0.0, tail=None):
    """Continuous-phase FSK, float32: `text` (through codes_of), or a sequence of raw codes of `nbits` bits, start-stop
    framed at `baud`; `lead` seconds of mark ahead and `tail` behind (default: 3 bits)."""
    fs, bit = float(fs), 1.0 / float(baud)
    codes = codes_of(text) if isinstance(text, str) else list(text)
    if tail is None:
        tail = 3 * bit
    ends, levels, t = [float(lead)], [True], float(lead)
    for m, bits in keying(codes, nbits, stop):
        t += bits * bit
        ends.append(t)
        levels.append(m)
    ends.append(t + float(tail))
    levels.append(True)
    n = int(round(ends[-1] * fs))
    which = np.searchsorted(np.asarray(ends), np.arange(n) / fs, side="right")          # the element a sample lies in
    f = np.where(np.asarray(levels)[np.minimum(which, len(levels) - 1)], float(mark), float(space))
    phase = 2.0 * np.pi * np.cumsum(f) / fs
    return (amp * np.sin(phase)).astype(np.float32)


__all__ = ["LETTERS", "FIGURES", "NUL", "LF", "SPACE", "CR", "FIGS", "LTRS", "BELL", "FRAMING_ERROR", "codes_of", "read_text",
           "rtty_config", "keying", "encode"]
