"""ACARS blocks beside the ACARS decoder bank (acars.py, include/ka9q_hip.h: kq_acars_*), plain Python: the characters'
parity, the block check, a block from its fields, MSK test traffic, the fields of a block the bank filed, the repair of a
block with a few parity errors and the reader of a bank's arenas.

This is ARINC 618's air-ground block as the open decoders read it, written down from memory; it has not been checked
against a signal off the air.  A block on the air: a pre-key of 2400 Hz, then + * SYN SYN SOH, mode, address (7), ack, label
(2), block id, STX and up to 220 characters of text (or neither), ETX or ETB, the block check (2 bytes, low first), DEL.
Characters are 7 bits, sent least significant bit first with bit 7 making the parity odd.  The block check is
CRC-16/KERMIT (0x8408 reflected, initial value 0, no final xor) over the bytes as sent, parity bits included, from the
mode character through ETX / ETB; run on over the two check bytes it leaves 0.  Bits run at 2400 a second; a bit equal to
the one before is sent as 2400 Hz and one that differs as 1200 Hz, the phase continuous.
"""
import collections
import itertools

import numpy as np

BAUD = 2400.0
PREAMBLE = (0x2b, 0x2a, 0x16, 0x16, 0x01)        # + * SYN SYN SOH, before parity
SOH, STX, ETX, ETB, DEL, NAK = 0x01, 0x02, 0x03, 0x17, 0x7f, 0x15
GOOD, ENDED_BY_ETB, OVERRUN = 1, 2, 4            # a record's flags
MAX_TEXT = 220

Block = collections.namedtuple("Block", "mode address ack label block_id text more msgno flight crc_ok parity_errors")
Record = collections.namedtuple("Record", "data length flags parity_errors sync_sample end_sample sync_c2 sync_e r2")


def parity(c):
    """a 7-bit character with bit 7 making the number of ones odd"""
    c &= 0x7f
    return c | (0 if bin(c).count("1") & 1 else 0x80)


def parity_ok(byte):
    return bin(byte & 0xff).count("1") & 1 == 1


def crc(data, start=0):
    """CRC-16/KERMIT of the bytes as sent"""
    r = start
    for b in bytes(data):
        r ^= b
        for _ in range(8):
            r = (r >> 1) ^ (0x8408 if r & 1 else 0)
    return r


def encode_block(mode="2", address=".N12345", ack=NAK, label="H1", block_id="1", text="", more=False):
    """the bytes of a block from the mode character through the block check, parity bits set.  address: 7 characters (shorter
    ones are filled with dots in front); ack: a character or its code; text: None for a block with no STX at all; more: the
    block ends with ETB, another follows"""
    def code(v):
        return ord(v) if isinstance(v, str) else int(v)
    if text is not None and len(text) > MAX_TEXT:
        raise ValueError("a block carries %d characters of text at the most" % MAX_TEXT)
    address = address.rjust(7, ".")
    if len(address) != 7 or len(label) != 2:
        raise ValueError("the address has 7 characters and the label 2")
    body = [code(mode)] + [ord(c) for c in address] + [code(ack)] + [ord(c) for c in label] + [code(block_id)]
    if text is not None and text != "":
        body += [STX] + [ord(c) for c in text]
    body.append(ETB if more else ETX)
    if any(c > 127 for c in body):
        raise ValueError("ACARS characters have 7 bits")
    sent = bytes(parity(c) for c in body)
    r = crc(sent)
    return sent + bytes((r & 0xff, r >> 8))


def block_bits(block, prekey_bits=64):
    """the bits on the air of one block (encode_block's bytes): pre-key, preamble, the block, DEL"""
    chars = [parity(c) for c in PREAMBLE] + list(bytes(block)) + [parity(DEL)]
    return [1] * int(prekey_bits) + [(c >> i) & 1 for c in chars for i in range(8)]


def modulate(blocks, fs, prekey_bits=64, amp=0.3, ppm=0.0, invert=False, start_phase=0.0, delay=0.0, lead=0, tail_bits=8,
             gap=0, info=None):
    """float32 audio of the blocks (each encode_block's bytes) one behind the other, each with its own pre-key: `lead`
    samples of silence, then the bits from `delay` (a fraction of a sample) on, `gap` samples of silence between two
    blocks, and tail_bits of 2400 Hz behind each DEL.  The sender's clock, bits and tones alike, is `ppm` parts in a
    million fast; start_phase is the tone's phase at the first bit, in radians; invert turns the audio over.  info: a list
    that gets, per block, the time in samples (a float) at which the last bit of SOH ends."""
    if isinstance(blocks, (bytes, bytearray)):
        blocks = [blocks]
    fs, fast = float(fs), 1.0 + float(ppm) * 1e-6
    per_bit = fs / (BAUD * fast)
    out, at = [np.zeros(int(lead), np.float32)], float(lead) + float(delay)
    for j, blk in enumerate(blocks):
        bits = np.array(block_bits(blk, prekey_bits) + [1] * int(tail_bits), np.int64)
        prev = np.concatenate(([1], bits[:-1]))
        turns = np.where(bits == prev, 1.0, 0.5)                       # of the tone per bit: 2400 / 2400, 1200 / 2400
        start = np.concatenate(([0.0], np.cumsum(turns)))
        first = sum(len(o) for o in out)
        frac = at - first                                              # the first bit starts this far into sample `first`
        n = int(np.ceil(frac + len(bits) * per_bit))
        u = (np.arange(n) - frac) / per_bit                            # the sender's time in bits
        k = np.clip(np.floor(u).astype(np.int64), 0, len(bits) - 1)
        x = float(amp) * np.sin(2.0 * np.pi * (start[k] + turns[k] * (u - k)) + float(start_phase))
        x[u < 0] = 0.0
        out.append((-x if invert else x).astype(np.float32))
        if info is not None:
            info.append(at + (int(prekey_bits) + 40) * per_bit)
        at = first + n + int(gap)
        if gap:
            out.append(np.zeros(int(gap), np.float32))
    return np.concatenate(out)


def parse(data, parity_errors=None):
    """the fields of a block (the bytes from mode through the block check): a Block.  For a downlink whose text begins with
    them, msgno is the message number (4 characters) and flight the flight id (6)"""
    data = bytes(data)
    if len(data) < 15:
        raise ValueError("a block has at least 15 bytes")
    body, bcs = data[:-2], data[-2:]
    ch = "".join(chr(b & 0x7f) for b in body)
    text = ch[13:-1] if len(ch) > 13 and ord(ch[12]) == STX else ""
    msgno = flight = None
    if ch[12:13] == chr(STX) and len(text) >= 10 and (ch[11].isdigit()) and text[:4].isalnum() and text[4:10].isalnum():
        msgno, flight = text[:4], text[4:10]
    bad = sum(not parity_ok(b) for b in body) if parity_errors is None else parity_errors
    return Block(ch[0], ch[1:8], ch[8], ch[9:11], ch[11], text, ord(ch[-1]) == ETB, msgno, flight, crc(body + bcs) == 0, bad)


def repair(data, parity_errors=None):
    """A block whose check does not close, with one to three characters of bad parity: one bit of each is flipped, every
    choice in turn, until the check closes.  Returns the mended bytes, or None.  (A block whose check closes comes back as
    it is.)"""
    data = bytearray(data)
    if crc(data) == 0:
        return bytes(data)
    bad = [i for i, b in enumerate(data[:-2]) if not parity_ok(b)]
    if not 1 <= len(bad) <= 3 or (parity_errors is not None and parity_errors != len(bad)):
        return None
    for flips in itertools.product(range(8), repeat=len(bad)):
        trial = bytearray(data)
        for i, bit in zip(bad, flips):
            trial[i] ^= 1 << bit
        if crc(trial) == 0:
            return bytes(trial)
    return None


def read_blocks(bank, slot=None, mend=True):
    """the blocks in a bank's arenas as (slot, Record, Block): of one slot, or of every slot that holds any.  A block whose
    check did not close is mended where repair() can (its Block then has crc_ok set and keeps the record's parity_errors)"""
    counts = bank.counts()
    out = []
    for s in ([slot] if slot is not None else np.nonzero(counts)[0]):
        for rec in bank.blocks(int(s), int(counts[s])):
            data = rec.data
            if mend and not rec.flags & GOOD and not rec.flags & OVERRUN:
                data = repair(data, rec.parity_errors) or data
            out.append((int(s), rec, parse(data, rec.parity_errors) if len(data) >= 15 else None))
    return out


__all__ = ["BAUD", "PREAMBLE", "SOH", "STX", "ETX", "ETB", "DEL", "NAK", "GOOD", "ENDED_BY_ETB", "OVERRUN", "MAX_TEXT", "Block",
           "Record", "parity", "parity_ok", "crc", "encode_block", "block_bits", "modulate", "parse", "repair", "read_blocks"]
