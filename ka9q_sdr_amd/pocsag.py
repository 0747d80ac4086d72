"""Host-side helpers for POCSAG pages as the pager decoder bank gives them (pag.PagBank.pages: a Page whose `words` are the
message words, 3 bytes each, big-endian: bits 19..0 the payload, bits 21..20 the error code, 3 = uncorrectable): the numeric
and the text alphabet, and an encoder that makes the codewords and line bits of a transmission (tools/bench_pag.py and the
tests generate their traffic with it).  The code itself -- constants, correction, deframer -- is defined in
include/ka9q_hip.h, kq_pag_*."""
import collections

import numpy as np

FSC = 0x7CD215D8
IDLE = 0x7A89C197
GENERATOR = 0x769                 # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
LOST, FULL, BAD = 1, 2, 4         # Page.flags
PREAMBLE_BITS = 576
BAUDS = (512, 1200, 2400)
NUMERIC = "0123456789*U -]["
UNCORRECTABLE = 3                 # a word's error code

Page = collections.namedtuple("Page", "ric function words flags errors end_sample")


def codeword(data21):
    """the 32-bit codeword of 21 data bits (flag and payload): BCH(31,21) check bits and even parity appended"""
    r = (data21 & 0x1FFFFF) << 10
    for i in range(30, 9, -1):
        if r >> i & 1:
            r ^= GENERATOR << (i - 10)
    w = ((data21 & 0x1FFFFF) << 10 | r) << 1
    return w | bin(w).count("1") & 1


def address_word(ric, function):
    """the address codeword of a 21-bit RIC; it belongs in frame ric & 7 of a batch"""
    return codeword((ric >> 3 & 0x3FFFF) << 2 | function & 3)


def message_word(payload20):
    return codeword(1 << 20 | payload20 & 0xFFFFF)


def _rev4(v):
    return (v & 1) << 3 | (v & 2) << 1 | (v & 4) >> 1 | (v & 8) >> 3


def numeric_payloads(text):
    """a numeric message as 20-bit payloads: five 4-bit digits a word, each sent LSB first, the last word filled with spaces"""
    digits = [NUMERIC.index(ch) for ch in text]
    digits += [NUMERIC.index(" ")] * (-len(digits) % 5)
    out = []
    for k in range(0, len(digits), 5):
        v = 0
        for d in digits[k:k + 5]:
            v = v << 4 | _rev4(d)
        out.append(v)
    return out


def alpha_payloads(text):
    """a text message as 20-bit payloads: 7-bit characters, each sent LSB first, running across the word boundaries; the last word is
    filled with zeros (NUL)"""
    bits = []
    for ch in text:
        c = ord(ch)
        if c > 127:
            raise ValueError("POCSAG text is 7-bit: %r" % ch)
        bits += [c >> i & 1 for i in range(7)]
    bits += [0] * (-len(bits) % 20)
    return [int("".join(map(str, bits[k:k + 20])), 2) for k in range(0, len(bits), 20)]


def _words(page):
    """(payload, error code) of every message word of a Page or of its `words` bytes"""
    raw = bytes(page.words if hasattr(page, "words") else page)
    if len(raw) % 3:
        raise ValueError("a page's words are 3 bytes each")
    vals = [int.from_bytes(raw[k:k + 3], "big") for k in range(0, len(raw), 3)]
    return [(v & 0xFFFFF, v >> 20 & 3) for v in vals]


def numeric(page):
    """the page in the numeric alphabet (0-9, *, U, space, -, ], [); the digits of an uncorrectable word read '?'; the
    spaces that fill the last word are stripped"""
    out = []
    for v, code in _words(page):
        if code == UNCORRECTABLE:
            out.append("?????")
        else:
            out.append("".join(NUMERIC[_rev4(v >> s & 15)] for s in (16, 12, 8, 4, 0)))
    return "".join(out).rstrip(" ")


def alpha(page):
    """the page as text: 7-bit characters, LSB first, across the word boundaries; a character that an uncorrectable word
    touches reads '?'; trailing NUL, ETX and EOT are stripped"""
    words = _words(page)
    bits, bad = [], []
    for v, code in words:
        bits += [v >> s & 1 for s in range(19, -1, -1)]
        bad += [code == UNCORRECTABLE] * 20
    chars = []
    for k in range(0, len(bits) - 6, 7):
        c = sum(b << i for i, b in enumerate(bits[k:k + 7]))
        chars.append("?" if any(bad[k:k + 7]) else chr(c))
    while chars and chars[-1] in "\x00\x03\x04":
        chars.pop()
    return "".join(chars)


def encode(pages, baud=1200):
    """One transmission: pages = [(ric, function, payloads)], payloads the 20-bit message words of each (numeric_payloads,
    alpha_payloads; none for a tone-only page).  Returns (codewords, bits): the words as sent, uint32, the FSC at the head of
    every batch of 16 among them, and the line bits, uint8 -- a preamble of 576 alternating bits, then every word MSB first.
    Each address goes in frame ric & 7 of a batch, its message words follow through frames and batches, IDLE fills the
    rest, and at least one IDLE follows the last page.  The bits do not depend on the rate: `baud` is checked, no more."""
    if baud not in BAUDS:
        raise ValueError("POCSAG runs at 512, 1200 or 2400 bit/s, not %r" % (baud,))
    body = []                                    # the codewords without the FSCs: batch k is body[16 k : 16 k + 16]
    for ric, function, payloads in pages:
        while len(body) % 16 != 2 * (ric & 7):
            body.append(IDLE)
        body.append(address_word(ric, function))
        body += [message_word(p) for p in payloads]
    body.append(IDLE)
    body += [IDLE] * (-len(body) % 16)
    words = []
    for k in range(0, len(body), 16):
        words += [FSC] + body[k:k + 16]
    words = np.array(words, np.uint32)
    bits = np.unpackbits(words.astype(">u4").view(np.uint8))
    pre = (np.arange(PREAMBLE_BITS) % 2 == 0).astype(np.uint8)
    return words, np.concatenate([pre, bits])


__all__ = ["FSC", "IDLE", "GENERATOR", "LOST", "FULL", "BAD", "NUMERIC", "UNCORRECTABLE", "PREAMBLE_BITS", "BAUDS", "Page",
           "codeword", "address_word", "message_word", "numeric_payloads", "alpha_payloads", "numeric", "alpha", "encode"]
