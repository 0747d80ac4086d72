"""Second-generation ALE (MIL-STD-188-141 Appendix A, FED-STD-1045) beside the ALE decoder bank (ale.py, include/ka9q_hip.h:
kq_ale_*), plain Python and numpy, no device: the preambles, the 38-character address set, the Gray map of the eight tones,
the extended Golay (24,12) code as a 4096-entry parity table, the word and its 49 symbols, phase-continuous 8-FSK for test
traffic, the bank's geometry for a sample rate, addresses and an individual call as words, and the reader of the bank's
events.

Written down from memory: no copy of the standard was at hand.  The tone plan (750 + 250 t Hz, 125 symbols a second), the
Gray map, the word (a 3-bit preamble and three 7-bit characters, highest bit first), the split into two Golay halves with
the second half's check bits inverted, the interleave A23 B23 .. A0 B0 with one stuff bit 0 and the threefold repeat are as
remembered.  The Golay check bits are the remainder of data x^11 by g(x) = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75)
followed by the overall parity bit; that this is a (24,12,8) code is checked (tests/test_ale_model.py), that it is the
standard's generator matrix bit for bit is NOT verified.  PARITY below is the single statement of the code, mirrored in
the kernel's table (ka9q_sdr_amd/csrc/kq_ale.hip builds it by the same rule), so a correction is a table swap.
"""
import numpy as np

PREAMBLES = ("DATA", "THRU", "TO", "TWAS", "FROM", "TIS", "CMD", "REP")
DATA, THRU, TO, TWAS, FROM, TIS, CMD, REP = range(8)
CHARSET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ@?"                  # the 38 characters of an address; @ stuffs
GRAY = (0b000, 0b001, 0b011, 0b010, 0b110, 0b111, 0b101, 0b100)     # tone t carries GRAY[t], the highest bit sent first
TONE = tuple(GRAY.index(v) for v in range(8))                        # and back
BAUD, F0, DF = 125.0, 750.0, 250.0
WORD_SYMBOLS = 49
HOLE = 1                                                             # an event's flag bit 0: a half could not be decoded
REPLACEMENT = "\ufffd"
GOLAY_POLY = 0xC75
UNCORRECTABLE = 4


def _parity(d):
    r = d << 11
    for i in range(22, 10, -1):
        if r >> i & 1:
            r ^= GOLAY_POLY << (i - 11)
    return r << 1 | (bin(d).count("1") + bin(r).count("1")) & 1


PARITY = np.array([_parity(d) for d in range(4096)], np.uint16)      # the 12 check bits of 12 data bits


def golay_parity():
    """the code: check bits by data bits, uint16 [4096]"""
    return PARITY


def _errors():
    """by syndrome: weight << 12 | the data bits of the one error pattern of weight <= 3 with it; 4 << 12 where none has"""
    out = np.full(4096, UNCORRECTABLE << 12, np.uint16)
    out[0] = 0
    bit = [1 << i for i in range(24)]
    for i in range(24):
        for j in range(i, 24):
            for k in range(j, 24):
                e = bit[i] | bit[j] | bit[k]                       # i == j or j == k give the lighter ones (more than once)
                out[int(PARITY[e >> 12]) ^ (e & 0xFFF)] = bin(e).count("1") << 12 | e >> 12
    return out


ERRORS = _errors()


def golay_encode(d):
    """12 data bits -> the 24-bit codeword, data first"""
    return int(d) << 12 | int(PARITY[int(d)])


def golay_decode(c):
    """a 24-bit word -> (data, weight): the nearest codeword's data and the bits that were corrected, or the word's own
    data bits and 4 where more than three are wrong"""
    d = int(c) >> 12
    e = int(ERRORS[int(PARITY[d]) ^ (int(c) & 0xFFF)])
    return d ^ (e & 0xFFF), e >> 12


def word(pre, chars):
    """the 24-bit word: a preamble (a name or 0..7) and three characters"""
    p = PREAMBLES.index(pre) if isinstance(pre, str) else int(pre)
    if len(chars) != 3 or any(ord(c) > 127 for c in chars) or not 0 <= p < 8:
        raise ValueError("a word is a preamble and three 7-bit characters: %r %r" % (pre, chars))
    return p << 21 | ord(chars[0]) << 14 | ord(chars[1]) << 7 | ord(chars[2])


def unword(w):
    """(preamble name, three characters) of a 24-bit word"""
    w = int(w)
    return PREAMBLES[w >> 21 & 7], "".join(chr(w >> s & 0x7F) for s in (14, 7, 0))


def word_bits(w):
    """the 49 bits of one copy, as an int, the first sent in bit 48: A23 B23 .. A0 B0 and the stuff bit"""
    a, b = golay_encode(int(w) >> 12 & 0xFFF), golay_encode(int(w) & 0xFFF) ^ 0xFFF
    out = 0
    for i in range(23, -1, -1):
        out = out << 2 | (a >> i & 1) << 1 | (b >> i & 1)
    return out << 1


def word_symbols(words):
    """the tones of the words, 49 each: every word's 49 bits three times over, three bits to a tone; uint8"""
    out = []
    for w in words:
        v = word_bits(w)
        v = v << 98 | v << 49 | v
        out += [TONE[v >> s & 7] for s in range(144, -1, -3)]
    return np.array(out, np.uint8)


def modulate_symbols(symbols, fs, f0=F0, df=DF, baud=BAUD, amp=0.3, lead=8, ppm=0.0, tail=4):
    """phase-continuous FSK, float32: `lead` symbol times of silence, the tones f0 + t df, `tail` of silence.  The
    sender's clock, symbols and tones alike, is `ppm` parts in a million fast."""
    sym = np.asarray(symbols, np.int64)
    fast = 1.0 + float(ppm) * 1e-6
    per = float(fs) / (float(baud) * fast)                           # samples to a symbol
    n0, n = int(round(lead * per)), int(np.ceil(len(sym) * per))
    i = np.minimum((np.arange(n) / per).astype(np.int64), len(sym) - 1)
    f = (float(f0) + float(df) * sym[i]) * fast
    ph = 2.0 * np.pi / float(fs) * (np.cumsum(f) - f)                # the phase at sample k: the frequencies before it
    out = np.zeros(n0 + n + int(round(tail * per)), np.float32)
    out[n0:n0 + n] = float(amp) * np.cos(ph)
    return out


def modulate(words, fs, f0=F0, df=DF, baud=BAUD, amp=0.3, lead=8, ppm=0.0, tail=4):
    """the words (24-bit ints) as 8-FSK; see modulate_symbols"""
    return modulate_symbols(word_symbols(words), fs, f0, df, baud, amp, lead, ppm, tail)


def ale_config(fs, baud=BAUD):
    """AleBank keywords for a sample rate: the frame (8 to 256 samples) nearest to eight in a symbol, with 8 to 32 in it"""
    fs = float(fs)
    block_len = min(max(int(round(fs / (8.0 * baud))), 8), 256)
    tb = round(256.0 * fs / (block_len * baud))
    if not 2048 <= tb <= 8192:
        raise ValueError("%g Hz does not suit %g symbols a second" % (fs, baud))
    return dict(block_len=block_len)


def address_words(pre, address):
    """an address as words: `pre` with its first three characters, then DATA and REP in turn with three more each; the
    last word is filled up with @"""
    address = address.upper()
    if not address or any(c not in CHARSET for c in address):
        raise ValueError("an address is made of 0-9 A-Z @ ?: %r" % address)
    address += "@" * (-len(address) % 3)
    pres = [pre] + [(DATA, REP)[k & 1] for k in range(len(address) // 3 - 1)]
    return [word(p, address[3 * k:3 * k + 3]) for k, p in enumerate(pres)]


def individual_call(to, frm, scans=1):
    """the words of an individual call: the called address's first word `scans` times over (the scanning call), the whole
    called address twice (the leading call), and TIS with the caller's"""
    t = address_words(TO, to)
    return t[:1] * int(scans) + t + t + address_words(TIS, frm)


def read(events):
    """the events of one slot (anything with `word` and `flags`) as (preamble name, address) pairs: a DATA or REP word
    goes on with the address before it, any other preamble begins one; the stuffing @ at an address's end is taken off.  A
    hole (a word that could not be decoded) stands as three U+FFFD in the address it falls into, or as a pair (None, ...)
    of its own"""
    out = []
    for e in events:
        hole = int(e.flags) & HOLE
        pre, chars = unword(e.word)
        if hole:
            pre, chars = None, REPLACEMENT * 3
        if out and (hole or pre in ("DATA", "REP")) and out[-1][0] is not None:
            out[-1][1] += chars
        else:
            out.append([pre, chars])
    return [(p, a.rstrip("@") if p != "CMD" else a) for p, a in out]


__all__ = ["PREAMBLES", "DATA", "THRU", "TO", "TWAS", "FROM", "TIS", "CMD", "REP", "CHARSET", "GRAY", "TONE", "BAUD", "F0", "DF",
           "WORD_SYMBOLS", "HOLE", "REPLACEMENT", "PARITY", "ERRORS", "UNCORRECTABLE", "golay_parity", "golay_encode",
           "golay_decode", "word", "unword", "word_bits", "word_symbols", "modulate_symbols", "modulate", "ale_config",
           "address_words", "individual_call", "read"]
