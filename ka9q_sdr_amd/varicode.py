"""The PSK31 alphabet beside the PSK decoder bank (psk.py, include/ka9q_hip.h: kq_psk_*), plain Python: Varicode as data, the
bank's geometry for a baud rate, shaped BPSK for test traffic, the reader of the bank's events and the frequency offset an
event's rotation stands for.

A character's code is its bits as sent, the first (always a 1) in the highest place: "e" is 0b11, a space 0b1.  Characters
are parted by two or more 0s; no code holds two 0s in a row.  On the air a 0 is a phase reversal and a 1 is none.
"""
import math

import numpy as np

# characters 0..127 in order
_TABLE = """
1010101011 1011011011 1011101101 1101110111 1011101011 1101011111 1011101111 1011111101 1011111111 11101111 11101 1101101111 1011011101 11111 1101110101 1110101011
1011110111 1011110101 1110101101 1110101111 1101011011 1101101011 1101101101 1101010111 1101111011 1101111101 1110110111 1101010101 1101011101 1110111011 1011111011 1101111111
1 111111111 101011111 111110101 111011011 1011010101 1010111011 101111111 11111011 11110111 101101111 111011111 1110101 110101 1010111 110101111
10110111 10111101 11101101 11111111 101110111 101011011 101101011 110101101 110101011 110110111 11110101 110111101 111101101 1010101 111010111 1010101111
1010111101 1111101 11101011 10101101 10110101 1110111 11011011 11111101 101010101 1111111 111111101 101111101 11010111 10111011 11011101 10101011
11010101 111011101 10101111 1101111 1101101 101010111 110110101 101011101 101110101 101111011 1010101101 111110111 111101111 111111011 1010111111 101101101
1011011111 1011 1011111 101111 101101 11 111101 1011011 101011 1101 111101011 10111111 11011 111011 1111 111
111111 110111111 10101 10111 101 110111 1111011 1101011 11011111 1011101 111010101 1010110111 110111011 1010110101 1011010111 1110110101
"""
VARICODE = tuple(_TABLE.split())                                     # by character, as strings of 0 and 1
assert len(VARICODE) == 128
CODES = tuple(int(s, 2) for s in VARICODE)                           # as the bank's events carry them
_CHAR = {c: chr(k) for k, c in enumerate(CODES)}

REPLACEMENT = "\ufffd"
FLAGGED = 1                                                          # an event's flag bit 0: more than 10 bits between gaps


def encode(text):
    """the bits of a text: every character's code and the gap of two 0s behind it"""
    out = []
    for ch in text:
        if ord(ch) > 127:
            raise ValueError("no Varicode for %r" % ch)
        out += [int(b) for b in VARICODE[ord(ch)]] + [0, 0]
    return out


def read_text(events):
    """the events of one slot (anything with `code` and `flags`) as text; a code that is no character's, or one that is
    flagged, becomes U+FFFD"""
    return "".join(REPLACEMENT if (int(e.flags) & FLAGGED) else _CHAR.get(int(e.code), REPLACEMENT) for e in events)


def psk_config(fs, baud):
    """PskBank keywords for a baud rate: the frame (8 to 256 samples) nearest to sixteen in a symbol, with 8 to 32 in it"""
    fs, baud = float(fs), float(baud)
    block_len = min(max(int(round(fs / (16.0 * baud))), 8), 256)
    tb = round(256.0 * fs / (block_len * baud))
    if not 2048 <= tb <= 8192:
        raise ValueError("%g Hz does not suit %g baud" % (fs, baud))
    return dict(block_len=block_len)


def modulate(text, fs, baud, pitch=1000.0, amp=0.3, lead=32, phase=0.0, ppm=0.0, tail=16, invert=False):
    """BPSK as PSK31 shapes it, float32: `text` (through encode), or a sequence of bits, behind `lead` reversals and ahead
    of `tail` symbols of carrier.  A 0 reverses the level at the symbol's centre against the one before.  Between two
    centres T = 1 / baud apart the envelope goes as cos(pi t / T) where the level reverses and is flat where it does not.
    `phase` is the carrier's at sample 0, in radians; the sender's clock, symbols and carrier alike, is `ppm` parts in a
    million fast; `invert` turns every level over."""
    bits = [0] * int(lead) + (encode(text) if isinstance(text, str) else [int(b) for b in text]) + [1] * int(tail)
    level = np.empty(len(bits) + 1)
    level[0] = -1.0 if invert else 1.0
    for i, b in enumerate(bits):
        level[i + 1] = level[i] if b else -level[i]
    fast = 1.0 + float(ppm) * 1e-6
    n = int(math.ceil(len(bits) / (float(baud) * fast) * float(fs)))
    u = np.arange(n) * (float(baud) * fast / float(fs))                # the sender's time in symbols; centre i is at u = i
    i = np.minimum(u.astype(np.int64), len(bits) - 1)
    a, b = level[i], level[i + 1]
    env = np.where(a == b, a, a * np.cos(np.pi * (u - i)))
    carrier = np.cos(2.0 * np.pi * float(pitch) * fast / float(fs) * np.arange(n) + float(phase))
    return (float(amp) * env * carrier).astype(np.float32)


def offset_hz(event, baud):
    """how far the signal lies above (positive) or below the slot's pitch, from an event's rot_r, rot_i: the turn per symbol
    that the decoder follows, times the baud rate.  The correlator's phase falls where the signal is above the pitch."""
    return -math.atan2(float(event.rot_i), float(event.rot_r)) / (2.0 * math.pi) * float(baud)


__all__ = ["VARICODE", "CODES", "REPLACEMENT", "FLAGGED", "encode", "read_text", "psk_config", "modulate", "offset_hz"]
