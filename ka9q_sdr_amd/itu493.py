"""GMDSS digital selective calling (ITU-R M.493) beside the DSC decoder bank (dsc.py, include/ka9q_hip.h: kq_dsc_*), plain
Python and numpy, no device: the ten-bit symbol, the places of a sequence with its phasing and its time diversity, the bits
and phase-continuous 2-FSK for test traffic, the bank's geometry for a sample rate, three kinds of message, and the reader
of the bank's events with the repair of a single hole from the error-check symbol.

Written down from memory: no copy of the Recommendation was at hand.  The symbol (seven information bits, the lowest first,
then the count of zeros among them as three bits, the highest first; 125 goes out as 1011111001), the phasing sequence (125
in the DX places 0, 2, .. 10; 111, 110, .. 104 in the RX places 1, 3, .. 15), message symbol i at the places 12 + 2 i and 17
+ 2 i, the repeated format specifier, the end-of-sequence symbols 117 (RQ), 122 (BQ) and 127, and the error-check symbol as
the XOR from the second format specifier through the end of sequence are as remembered.  NOT verified: which audio tone is
state B on which sideband (MARK and SPACE below are a guess that the decoder does not depend on: it takes the complement
as well); what the DX places carry while the last RX copies go out (the end-of-sequence symbol here); the field layouts of
distress_alert, all_ships and individual_call, their category, nature and telecommand numbers, and the packing of positions
and frequencies; the expansion sequences of later revisions.  Nothing here has met a signal off the air.
"""
import numpy as np

DX_PHASING = 125
RX_PHASING = tuple(range(111, 103, -1))                              # at the places 1, 3, .. 15
RQ, BQ, END = 117, 122, 127                                          # end of sequence: acknowledgement wanted, given, neither
EOS = (RQ, BQ, END)
DISTRESS, ALL_SHIPS, INDIVIDUAL = 112, 116, 120                      # format specifiers
ROUTINE, SAFETY, URGENCY, DISTRESS_CATEGORY = 100, 108, 110, 112     # categories
NO_INFORMATION = 126
J3E, F3E = 109, 100                                                  # first telecommands: SSB and FM telephony
UNDESIGNATED = 107                                                   # nature of distress
HOLE = 0xFF                                                          # an event's byte for a symbol neither copy gave
CHECK, TRUNCATED, LOST, INVERTED = 1, 2, 4, 8                        # an event's flag bits
MAX_SYMBOLS = 64
BAUD, MARK, SPACE = 100.0, 1785.0, 1615.0                            # HF / MF on a USB channel 1700 Hz below the assigned one
VHF_BAUD, VHF_MARK, VHF_SPACE = 1200.0, 1300.0, 2100.0


def encode_symbol(v):
    """the ten bits of symbol v (0..127) as an int, the first sent in bit 9"""
    v = int(v)
    if not 0 <= v < 128:
        raise ValueError("a symbol is 0..127: %r" % v)
    info = int("{:07b}".format(v)[::-1], 2)                          # the lowest bit first
    return info << 3 | (7 - bin(v).count("1"))


def decode_symbol(w):
    """the value of a ten-bit word, or None where its count of zeros does not agree"""
    w = int(w) & 1023
    if 7 - bin(w >> 3).count("1") != (w & 7):
        return None
    return int("{:07b}".format(w >> 3)[::-1], 2)


def check_symbol(symbols):
    """the error-check symbol of a message given from its first format specifier through its end of sequence: the XOR of
    all but the first"""
    out = 0
    for v in list(symbols)[1:]:
        out ^= int(v)
    return out


def message(fmt, body, eos=END):
    """the message symbols: the format specifier twice, the body, the end of sequence and the error-check symbol"""
    if eos not in EOS:
        raise ValueError("an end of sequence is one of %r" % (EOS,))
    sym = [int(fmt), int(fmt)] + [int(v) for v in body] + [int(eos)]
    if any(not 0 <= v < 128 for v in sym) or any(v in EOS for v in sym[:-1]):
        raise ValueError("message symbols are 0..127, and none before the end is an end of sequence: %r" % (sym,))
    sym.append(check_symbol(sym))
    if len(sym) > MAX_SYMBOLS:
        raise ValueError("%d symbols: a message has %d at the most" % (len(sym), MAX_SYMBOLS))
    return sym


def sequence(symbols):
    """the symbol of every place, 2 n + 16 of them for n message symbols: the phasing, then message symbol i at the DX
    place 12 + 2 i and the RX place 17 + 2 i; the two DX places behind the last message symbol repeat the end of sequence"""
    sym = [int(v) for v in symbols]
    n = len(sym)
    fill = sym[-2] if n >= 2 else END
    out = []
    for p in range(2 * n + 16):
        if p & 1:
            out.append(RX_PHASING[p >> 1] if p <= 15 else sym[(p - 17) >> 1])
        else:
            i = (p - 12) >> 1
            out.append(DX_PHASING if p <= 10 else sym[i] if i < n else fill)
    return out


def place_bits(places, dots=20):
    """the dot pattern (20 bits, or 200 on HF / MF where receivers scan) and the ten bits of every place's symbol, uint8"""
    if dots not in (20, 200):
        raise ValueError("a dot pattern is 20 or 200 bits")
    out = [(k + 1) & 1 for k in range(dots)]
    for v in places:
        w = encode_symbol(v)
        out += [w >> s & 1 for s in range(9, -1, -1)]
    return np.array(out, np.uint8)


def bits(symbols, dots=20):
    """the bits of a message's sequence: place_bits(sequence(symbols), dots)"""
    return place_bits(sequence(symbols), dots)


def modulate(bit_values, fs, baud=BAUD, mark=MARK, space=SPACE, amp=0.3, lead=8, ppm=0.0, tail=4):
    """phase-continuous FSK, float32: `lead` bit times of silence, state B (1) at `mark` and Y (0) at `space`, `tail` of
    silence.  The sender's clock, bits and tones alike, is `ppm` parts in a million fast."""
    b = np.asarray(bit_values, np.int64)
    fast = 1.0 + float(ppm) * 1e-6
    per = float(fs) / (float(baud) * fast)                           # samples to a bit
    n0, n = int(round(lead * per)), int(np.ceil(len(b) * per))
    i = np.minimum((np.arange(n) / per).astype(np.int64), len(b) - 1)
    f = np.where(b[i] != 0, float(mark), float(space)) * fast
    ph = 2.0 * np.pi / float(fs) * (np.cumsum(f) - f)                # the phase at sample k: the frequencies before it
    out = np.zeros(n0 + n + int(round(tail * per)), np.float32)
    out[n0:n0 + n] = float(amp) * np.cos(ph)
    return out


def dsc_config(fs, baud=BAUD):
    """DscBank keywords for a sample rate: the frame (8 to 256 samples) nearest to ten in a bit, with 8 to 32 in it"""
    fs = float(fs)
    block_len = min(max(int(round(fs / (10.0 * baud))), 8), 256)
    tb = round(256.0 * fs / (block_len * baud))
    if not 2048 <= tb <= 8192:
        raise ValueError("%g Hz does not suit %g baud" % (fs, baud))
    return dict(block_len=block_len)


def digits_symbols(digits):
    """decimal digits, two to a symbol (an even count)"""
    d = str(digits)
    if len(d) % 2 or not d.isdigit():
        raise ValueError("an even count of decimal digits: %r" % (digits,))
    return [int(d[k:k + 2]) for k in range(0, len(d), 2)]


def mmsi_symbols(mmsi):
    """a nine-digit identity as five symbols: its digits and a trailing 0, two BCD digits to a symbol"""
    d = "%09d" % int(mmsi)
    if len(d) != 9:
        raise ValueError("an MMSI has nine digits: %r" % (mmsi,))
    return digits_symbols(d + "0")


def symbols_mmsi(sym):
    """and back; None where a symbol is no pair of digits"""
    if len(sym) != 5 or any(v is None or not 0 <= v <= 99 for v in sym):
        return None
    return "".join("%02d" % v for v in sym)[:9]


def individual_call(to, frm, category=ROUTINE, telecommand=(J3E, NO_INFORMATION), frequency=(NO_INFORMATION,) * 6, eos=RQ):
    """format 120 (as remembered): the called identity, the category, the caller's identity, two telecommands, the
    frequency or position message (six symbols; () leaves it out for short test traffic)"""
    return message(INDIVIDUAL, mmsi_symbols(to) + [category] + mmsi_symbols(frm) + list(telecommand) + list(frequency), eos)


def all_ships(frm, category=SAFETY, telecommand=(J3E, NO_INFORMATION), frequency=(NO_INFORMATION,) * 6):
    """format 116 (as remembered): the category, the caller's identity, two telecommands, the frequency message"""
    return message(ALL_SHIPS, [category] + mmsi_symbols(frm) + list(telecommand) + list(frequency), END)


def distress_alert(frm, nature=UNDESIGNATED, position="9999999999", time="8888", telecommand=J3E):
    """format 112 (as remembered): the identity in distress, the nature, the position (ten digits: the quadrant, the
    latitude ddmm, the longitude dddmm; all 9 where unknown), the time hhmm UTC (8888 where unknown), the telecommand for
    the traffic that follows"""
    return message(DISTRESS, mmsi_symbols(frm) + [nature] + digits_symbols(position) + digits_symbols(time) + [telecommand], END)


def event_symbols(event):
    """the symbols of an event as a list, None where unresolved"""
    raw = bytes(event.sym)[:int(event.nsym)]
    mask = int(event.hole_mask)
    return [None if mask >> i & 1 else int(v) for i, v in enumerate(raw)]


def repair(event):
    """the event with a single hole rebuilt on the host: the first format specifier from the second (or the second from
    the first), any other symbol -- the error-check symbol included -- as the XOR that makes the check come out.  Only a
    message that ended by its end of sequence can be mended; any other event comes back as it is."""
    flags = int(event.flags)
    sym = event_symbols(event)
    if int(event.holes) != 1 or flags & (TRUNCATED | LOST) or len(sym) < 4 or sym[-2] not in EOS:
        return event
    h = sym.index(None)
    if h == 0:
        sym[0] = sym[1]
    else:
        sym[h] = 0
        sym[h] = check_symbol(sym)                                   # the XOR of all from symbol 1 on is 0
    if sym[0] != sym[1]:
        return event
    raw = bytes(sym) + bytes(event.sym)[len(sym):]
    return event._replace(sym=raw, flags=flags & ~CHECK, holes=0, hole_mask=0)


def parse(event):
    """an event (anything with sym, nsym, flags, holes, hole_mask) as a dict: kind, the fields of the three kinds built
    here (identities as nine-digit strings), symbols (None where unresolved), ok (the check held), inverted, eos"""
    sym, flags = event_symbols(event), int(event.flags)
    out = dict(kind=None, symbols=sym, ok=not flags & (CHECK | TRUNCATED | LOST), inverted=bool(flags & INVERTED),
               truncated=bool(flags & TRUNCATED), lost=bool(flags & LOST), holes=int(event.holes), eos=None)
    whole = not flags & (TRUNCATED | LOST) and len(sym) >= 4
    body = sym[2:-2] if whole else sym[2:]
    if whole:
        out["eos"] = sym[-2]
    fmt = sym[0] if sym and sym[0] is not None else (sym[1] if len(sym) > 1 else None)
    out["format"] = fmt
    if fmt == INDIVIDUAL and len(body) >= 13:
        out.update(kind="individual", to=symbols_mmsi(body[0:5]), category=body[5], frm=symbols_mmsi(body[6:11]),
                   telecommand=tuple(body[11:13]), frequency=tuple(body[13:]))
    elif fmt == ALL_SHIPS and len(body) >= 8:
        out.update(kind="all_ships", category=body[0], frm=symbols_mmsi(body[1:6]), telecommand=tuple(body[6:8]),
                   frequency=tuple(body[8:]))
    elif fmt == DISTRESS and len(body) >= 14:
        digits = lambda part: None if any(v is None or v > 99 for v in part) else "".join("%02d" % v for v in part)
        out.update(kind="distress", frm=symbols_mmsi(body[0:5]), nature=body[5], position=digits(body[6:11]),
                   time=digits(body[11:13]), telecommand=body[13])
    return out


def read(events):
    """the events of one slot as parsed messages, each mended first where a single hole allows it"""
    return [parse(repair(e)) for e in events]


__all__ = ["DX_PHASING", "RX_PHASING", "RQ", "BQ", "END", "EOS", "DISTRESS", "ALL_SHIPS", "INDIVIDUAL", "ROUTINE", "SAFETY",
           "URGENCY", "DISTRESS_CATEGORY", "NO_INFORMATION", "J3E", "F3E", "UNDESIGNATED", "HOLE", "CHECK", "TRUNCATED", "LOST",
           "INVERTED", "MAX_SYMBOLS", "BAUD", "MARK", "SPACE", "VHF_BAUD", "VHF_MARK", "VHF_SPACE", "encode_symbol",
           "decode_symbol", "check_symbol", "message", "sequence", "place_bits", "bits", "modulate", "dsc_config", "digits_symbols",
           "mmsi_symbols", "symbols_mmsi", "individual_call", "all_ships", "distress_alert", "event_symbols", "repair", "parse",
           "read"]
