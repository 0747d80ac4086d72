"""EAS / SAME (Specific Area Message Encoding; 47 CFR 11.31, NWS Instruction 10-1712) beside the SAME decoder bank (same.py,
include/ka9q_hip.h: kq_same_*), plain Python and numpy, no device: the header's text and its parse, a burst's bits,
phase-continuous AFSK for test audio with the bit edges at exact fractional sample positions, the bank's geometry for a
sample rate, the reader of the bank's events, and the bitwise vote of two of three over the repeats.

Written down from memory: no copy of the rule or of the Instruction was at hand.  That covers the tone frequencies and the
bit rate, the preamble byte and its count, the bit order, the grammar of the header, the originator codes and the EVENTS
table, which is incomplete as well.  Nothing here has met a signal off the air.
"""
import collections
import re

import numpy as np

BAUD, MARK, SPACE = 3125.0 / 6.0, 6250.0 / 3.0, 1562.5             # a bit is 1.92 ms: four cycles of mark, three of space
PREAMBLE, PREAMBLE_BYTES = 0xAB, 16
ATTENTION = dict(broadcast=(853.0, 960.0), weather=(1050.0,))
START, BAD, END = 1, 2, 4                                            # an event's flag bits
COMPLETE, LOST, LENGTH = 1, 2, 3                                     # an END event's code
MAX_LOCATIONS, MAX_BYTES = 31, 252
EOM = "NNNN"

ORIGINATORS = dict(EAS="broadcast station or cable system", CIV="civil authorities", WXR="National Weather Service",
                   PEP="primary entry point system")
# FROM MEMORY AND INCOMPLETE: a code that is not here passes through parse() as it is
EVENTS = dict(
    EAN="Emergency Action Notification", EAT="Emergency Action Termination", NIC="National Information Center",
    NPT="National Periodic Test", RMT="Required Monthly Test", RWT="Required Weekly Test", ADR="Administrative Message",
    AVA="Avalanche Watch", AVW="Avalanche Warning", BZW="Blizzard Warning", CAE="Child Abduction Emergency",
    CDW="Civil Danger Warning", CEM="Civil Emergency Message", CFA="Coastal Flood Watch", CFW="Coastal Flood Warning",
    DMO="Practice / Demo Warning", DSW="Dust Storm Warning", EQW="Earthquake Warning", EVI="Evacuation Immediate",
    EWW="Extreme Wind Warning", FFA="Flash Flood Watch", FFS="Flash Flood Statement", FFW="Flash Flood Warning",
    FLA="Flood Watch", FLS="Flood Statement", FLW="Flood Warning", FRW="Fire Warning", HLS="Hurricane Statement",
    HMW="Hazardous Materials Warning", HUA="Hurricane Watch", HUW="Hurricane Warning", HWA="High Wind Watch",
    HWW="High Wind Warning", LAE="Local Area Emergency", LEW="Law Enforcement Warning", NMN="Network Message Notification",
    NUW="Nuclear Power Plant Warning", RHW="Radiological Hazard Warning", SMW="Special Marine Warning",
    SPS="Special Weather Statement", SPW="Shelter in Place Warning", SSA="Storm Surge Watch", SSW="Storm Surge Warning",
    SVA="Severe Thunderstorm Watch", SVR="Severe Thunderstorm Warning", SVS="Severe Weather Statement",
    TOA="Tornado Watch", TOE="911 Telephone Outage Emergency", TOR="Tornado Warning", TRA="Tropical Storm Watch",
    TRW="Tropical Storm Warning", TSA="Tsunami Watch", TSW="Tsunami Warning", VOW="Volcano Warning",
    WSA="Winter Storm Watch", WSW="Winter Storm Warning")

Header = collections.namedtuple("Header", "org event event_name locations purge issued station")
Burst = collections.namedtuple("Burst", "kind text data bad reason errs start_sample end_sample")
Alert = collections.namedtuple("Alert", "text copies start_sample")
_GRAMMAR = re.compile(r"ZCZC-([A-Z]{3})-([A-Z0-9]{3})((?:-[0-9]{6}){1,%d})\+([0-9]{4})-([0-9]{7})-([\x20-\x7E]{8})-" % MAX_LOCATIONS)


def header(org, event, locations, purge, issued, station):
    """ZCZC-ORG-EEE-PSSCCC[-PSSCCC...]+TTTT-JJJHHMM-LLLLLLLL-.  locations: 1 to 31 codes PSSCCC (six digits, or an int);
    purge: (hours, minutes) or "hhmm"; issued: (day of the year, hour, minute) in UTC, or "JJJHHMM"; station: up to eight
    characters, a `-` in it written `/`, filled with spaces"""
    locations = ["%06d" % v if isinstance(v, int) else str(v) for v in locations]
    if not 1 <= len(locations) <= MAX_LOCATIONS:
        raise ValueError("a header holds 1 to %d location codes, not %d" % (MAX_LOCATIONS, len(locations)))
    purge = purge if isinstance(purge, str) else "%02d%02d" % tuple(purge)
    issued = issued if isinstance(issued, str) else "%03d%02d%02d" % tuple(issued)
    station = str(station).replace("-", "/")
    if len(station) > 8:
        raise ValueError("a station has eight characters at the most: %r" % station)
    text = "ZCZC-%s-%s-%s+%s-%s-%-8s-" % (org, event, "-".join(locations), purge, issued, station)
    if len(text) > MAX_BYTES:
        raise ValueError("a header has %d bytes at the most, not %d" % (MAX_BYTES, len(text)))
    parse(text)
    return text


def parse(text):
    """the fields of a header, a Header: org, event, event_name (the code itself where EVENTS does not know it), locations
    (the codes PSSCCC as strings), purge (minutes), issued (day of the year, hour, minute), station (as sent, spaces
    stripped).  ValueError on a text outside the grammar"""
    m = _GRAMMAR.fullmatch(text)
    if not m:
        raise ValueError("not a SAME header: %r" % (text,))
    org, event, locs, purge, issued, station = m.groups()
    if org not in ORIGINATORS:
        raise ValueError("originator %r is none of %s" % (org, ", ".join(ORIGINATORS)))
    if len(text) > MAX_BYTES:
        raise ValueError("a header has %d bytes at the most, not %d" % (MAX_BYTES, len(text)))
    day, hour, minute = int(issued[:3]), int(issued[3:5]), int(issued[5:])
    if not (1 <= day <= 366 and hour < 24 and minute < 60 and int(purge[2:]) < 60):
        raise ValueError("no such time: +%s-%s" % (purge, issued))
    return Header(org, event, EVENTS.get(event, event), locs[1:].split("-"), 60 * int(purge[:2]) + int(purge[2:]),
                  (day, hour, minute), station.strip())


def burst(text):
    """the bits of one burst, uint8: 16 bytes of preamble 0xAB, then the text, every byte's least significant bit first"""
    data = bytes([PREAMBLE]) * PREAMBLE_BYTES + text.encode("ascii")
    return np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")


def afsk(bit_values, fs, start=0.0, baud=BAUD, mark=MARK, space=SPACE, amp=0.3):
    """(n0, samples): phase-continuous AFSK of the bits, the first bit's edge at the fractional sample position `start` and
    every later edge at start + j fs / baud exactly; the samples are those at the integers n0 .. inside the burst, float64.
    The phase at a sample is the integral of the frequency from `start` to it, so a bit edge between two samples turns
    the frequency over there and not at a sample"""
    b = np.asarray(bit_values, np.int64)
    per = float(fs) / float(baud)
    n0, n1 = int(np.ceil(start)), int(np.ceil(start + len(b) * per))
    x = np.arange(n0, n1, dtype=np.float64) - start                 # time since the first edge, in samples
    i = np.minimum((x / per).astype(np.int64), len(b) - 1)
    f = np.where(b != 0, float(mark), float(space))
    before = np.concatenate([[0.0], np.cumsum(f)[:-1]]) * per        # cycles * fs up to each bit's leading edge
    return n0, float(amp) * np.cos(2.0 * np.pi / float(fs) * (before[i] + f[i] * (x - i * per)))


def modulate(text, fs, attention=None, attention_seconds=8.0, eom=True, ppm=0.0, amp=0.3, lead=0.25, gap=1.0, tail=0.25,
             repeats=3):
    """test audio of one alert, float32: `lead` seconds of silence, the burst of `text` `repeats` times with `gap` seconds
    between; then, with attention "broadcast" (853 + 960 Hz) or "weather" (1050 Hz), `gap`, the attention signal and `gap`;
    then, with eom, the burst of NNNN `repeats` times; `tail` of silence.  The sender's clock -- bits, tones and pauses
    alike -- is `ppm` parts in a million fast"""
    fast = 1.0 + float(ppm) * 1e-6
    fs_tx = float(fs) / fast                                         # the receiver's samples in a second of the sender's
    parts, at = [], float(lead) * fs_tx
    for part, what in enumerate((text, EOM) if eom else (text,)):
        b = burst(what)
        for _ in range(repeats):
            parts.append(afsk(b, fs_tx, at, amp=amp))
            at += len(b) * fs_tx / BAUD + float(gap) * fs_tx
        if part == 0 and attention is not None:
            n0, n = int(np.ceil(at)), int(float(attention_seconds) * fs_tx)
            t = np.arange(n0, n0 + n, dtype=np.float64) / fs_tx
            tones = ATTENTION[attention]
            parts.append((n0, sum(float(amp) / len(tones) * np.cos(2.0 * np.pi * f * t) for f in tones)))
            at = n0 + n + float(gap) * fs_tx
    out = np.zeros(int(np.ceil(at - float(gap) * fs_tx + float(tail) * fs_tx)), np.float64)
    for n0, v in parts:
        out[n0:n0 + len(v)] += v
    return out.astype(np.float32)


def same_config(fs, baud=BAUD):
    """SameBank keywords for a sample rate: the frame (8 samples at the least) nearest to ten in a bit, with 8 to 32 in it"""
    fs = float(fs)
    block_len = min(max(int(round(fs / (10.0 * baud))), 8), 256)
    tb = round(256.0 * fs / (block_len * baud))
    if not 2048 <= tb <= 8192:
        raise ValueError("%g Hz does not suit %g baud: resample to 48 kHz first" % (fs, baud))
    return dict(block_len=block_len)


def read(events):
    """the bursts of one slot's events (anything with code, flags, index, errs and end_sample), in order, each a Burst: kind
    ("Z" a header, "N" an end of message), text (ZCZC and the bytes read, a bad byte as `?`; NNNN), data (the bytes as
    read, ahead of them ZCZC or NNNN), bad (the positions in text of the bad bytes), reason (the END event's code; 0 for an
    end of message and for a burst still open), errs (wrong bits among the 48 of the sync), start_sample and end_sample"""
    out, cur = [], None

    def close(reason, end):
        nonlocal cur
        if cur is not None:
            kind, data, bad, errs, start, last = cur
            out.append(Burst(kind, "".join(chr(b) if 0x20 <= b <= 0x7E else "?" for b in data), bytes(data), bad, reason, errs,
                             start, end if end is not None else last))
        cur = None

    for e in events:
        code, flags, at = int(e.code), int(e.flags), int(e.end_sample)
        if flags & START:
            close(0, None)
            cur = [chr(code), list(b"ZCZC" if code == ord("Z") else b"NNNN"), [], int(e.errs), at, at]
            if code != ord("Z"):
                close(0, at)
        elif flags & END:
            close(code, at)
        elif cur is not None:
            if flags & BAD:
                cur[2].append(len(cur[1]))
            cur[1].append(code & 255)
            cur[5] = at
    close(0, None)
    return out


def clip(text):
    """the text up to the grammar's own end, the third dash behind the `+`, where it has one"""
    at = text.find("+")
    for _ in range(3):
        if at < 0:
            return text
        at = text.find("-", at + 1)
    return text[:at + 1] if at >= 0 else text


def _vote3(a, b, c):
    return bytes((x & y) | (y & z) | (x & z) for x, y, z in zip(a, b, c))


def vote(bursts, fs, within=8.0):
    """the headers of an alert's repeats, each an Alert (text, copies, start_sample): header bursts that start within
    `within` seconds of the first of them are one alert's.  Of three, the bitwise two of three over the bytes that at least
    two of them hold (where only two hold a byte, it is taken where they agree, else it is `?`), cut at the grammar's
    end; of two, their text where they agree up to the grammar's end; one alone gives nothing"""
    heads = [b for b in bursts if b.kind == "Z"]
    out, k = [], 0
    while k < len(heads):
        group = [b for b in heads[k:k + 3] if b.start_sample - heads[k].start_sample <= within * float(fs)]
        k += len(group)
        data = sorted((b.data for b in group), key=len)
        if len(group) == 3:
            n2, n3 = len(data[1]), len(data[0])                     # held by two at the least, and by all three
            both = bytes(x if x == y else ord("?") for x, y in zip(data[1][n3:n2], data[2][n3:n2]))
            voted = _vote3(*(d[:n3] for d in data)) + both
            text = "".join(chr(v) if 0x20 <= v <= 0x7E else "?" for v in voted)
            out.append(Alert(clip(text), 3, group[0].start_sample))
        elif len(group) == 2 and clip(group[0].text) == clip(group[1].text) and "?" not in clip(group[0].text):
            out.append(Alert(clip(group[0].text), 2, group[0].start_sample))
    return out


__all__ = ["BAUD", "MARK", "SPACE", "PREAMBLE", "PREAMBLE_BYTES", "ATTENTION", "START", "BAD", "END", "COMPLETE", "LOST", "LENGTH",
           "MAX_LOCATIONS", "MAX_BYTES", "EOM", "ORIGINATORS", "EVENTS", "Header", "Burst", "Alert", "header", "parse", "burst",
           "afsk", "modulate", "same_config", "read", "clip", "vote"]
