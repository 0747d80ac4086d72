"""Host-side helpers for AIS frames as the FSK decoder bank gives them (fsk.FskBank.frames: body + the two FCS bytes, each
byte filled LSB first from the line): the message bits, the !AIVDM sentences and the position of the common reports."""
import numpy as np


def ais_payload_bits(frame):
    """the frame without its FCS as message bits, uint8 0 / 1: AIS sends each byte LSB first, so the message's bit order is
    every byte from its MSB down"""
    return np.unpackbits(np.frombuffer(bytes(frame[:-2]), np.uint8))


def _armour(v):
    return chr(v + 48 if v < 40 else v + 56)


def _sentence(body):
    cs = 0
    for ch in body:
        cs ^= ord(ch)
    return "!%s*%02X" % (body, cs)


def ais_nmea(frame, channel="A", seq=1):
    """the !AIVDM sentences of a frame, a list: one for payloads up to 168 bits, else parts of 60 characters numbered with
    the sequence id `seq`.  Six bits per character, the last one filled up with zeros and the fill count after the payload;
    the checksum is the XOR of the characters between '!' and '*'."""
    bits = ais_payload_bits(frame)
    fill = (-len(bits)) % 6
    bits = np.concatenate([bits, np.zeros(fill, np.uint8)])
    vals = bits.reshape(-1, 6) @ (1 << np.arange(5, -1, -1))
    text = "".join(_armour(int(v)) for v in vals)
    if len(bits) - fill <= 168:
        return [_sentence("AIVDM,1,1,,%s,%s,%d" % (channel, text, fill))]
    parts = [text[i:i + 60] for i in range(0, len(text), 60)]
    return [_sentence("AIVDM,%d,%d,%d,%s,%s,%d" % (len(parts), k + 1, seq, channel, p, fill if k == len(parts) - 1 else 0))
            for k, p in enumerate(parts)]


def ais_bits_from_nmea(sentence):
    """the message bits of one !AIVDM sentence (checksum verified), uint8 0 / 1"""
    body, cs = sentence[1:].split("*")
    want = 0
    for ch in body:
        want ^= ord(ch)
    if want != int(cs, 16):
        raise ValueError("checksum %s, computed %02X" % (cs, want))
    f = body.split(",")
    vals = [ord(ch) - 48 - (8 if ord(ch) - 48 > 40 else 0) for ch in f[5]]
    bits = ((np.array(vals)[:, None] >> np.arange(5, -1, -1)) & 1).astype(np.uint8).reshape(-1)
    return bits[:len(bits) - int(f[6])]


def _field(bits, at, n, signed=False):
    v = 0
    for b in bits[at:at + n]:
        v = (v << 1) | int(b)
    if signed and v >> (n - 1):
        v -= 1 << n
    return v


def ais_position(frame):
    """type, mmsi, longitude and latitude (degrees), course (degrees) and heading of a position report (message types 1, 2,
    3 and 18), or None for any other message"""
    bits = ais_payload_bits(frame)
    if len(bits) < 6:
        return None
    mtype = _field(bits, 0, 6)
    if mtype in (1, 2, 3):
        lon, lat, cog, hdg = 61, 89, 116, 128
    elif mtype == 18:
        lon, lat, cog, hdg = 57, 85, 112, 124
    else:
        return None
    if len(bits) < hdg + 9:
        return None
    return dict(type=mtype, mmsi=_field(bits, 8, 30), longitude=_field(bits, lon, 28, True) / 600000.0,
                latitude=_field(bits, lat, 27, True) / 600000.0, course=_field(bits, cog, 12) / 10.0,
                heading=_field(bits, hdg, 9))


__all__ = ["ais_payload_bits", "ais_nmea", "ais_bits_from_nmea", "ais_position"]
