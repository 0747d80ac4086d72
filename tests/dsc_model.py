"""The DSC decoder of include/ka9q_hip.h (kq_dsc_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, two correlators whose phases are functions of the sample index alone, a sliding window
one bit long over the frames' reduced sums (rtty_model's front half), the early / centre / late clock on the larger of
the two powers with its push from half a bit out, the levels and the gate, the 64-bit register, the attempt on the phasing sequence, and the message resolved
from its DX and RX copies up to its end.  The frame sums are taken in int64 (they stay below 2^38) and everything from the
shifts on in Python ints: there is no float after the quantiser.  The bit length becomes an integer (tb) before any sample
is seen, by the header's formula in double."""
import collections

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
M64 = (1 << 64) - 1
MAX_SYMBOLS = 64
W125 = 0b1011111001
CHECK, TRUNCATED, LOST, INVERTED = 1, 2, 4, 8
Event = collections.namedtuple("Event", "sym nsym flags holes from_rx hole_mask sync_sample end_sample sig nse")
STATUS = ("frames", "ph", "t", "bit", "nbits", "synced", "bitpos", "events", "dropped", "syncs", "aborted", "reserved", "sig",
          "nse", "ee", "el", "ec", "pe", "hi", "lo", "r", "sum", "acc", "inverted", "place", "nsym", "nres", "holes", "from_rx", "run",
          "ecc", "eos", "reserved2", "hole_mask", "sync_sample", "msg")

cos_table, dsc_inc, bit_length, window = gm.cos_table, gm.inc, gm.period, gm.window


def is_symbol(w):
    return 7 - bin(w >> 3).count("1") == (w & 7)


def value_of(w):
    """the seven bits of w >> 3 reversed"""
    return sum((w >> (9 - i) & 1) << i for i in range(7))


def word_of(v):
    return sum((v >> i & 1) << (9 - i) for i in range(7)) | (7 - bin(v & 127).count("1"))


def phasing(x, acq):
    """the header's step 4 on x: the place of the latest symbol, or -1"""
    s0, s1, s2, s3 = x & 1023, x >> 10 & 1023, x >> 20 & 1023, x >> 30 & 1023
    if not is_symbol(s0):
        return -1
    v = value_of(s0)
    if not 104 <= v <= 110:
        return -1
    m = int(s2 == word_of(v + 1)) + int(v >= 106 and s1 == W125) + int(v >= 105 and s3 == W125)
    return 2 * (111 - v) + 1 if m >= acq else -1


class DscModel(gm.GridModel):
    """one slot.  table, incs, tb: the bank's own (kq_dsc_get_table, kq_dsc_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it).  gate=False leaves the gate open, nudge=False leaves out step 1's push from half a bit
    out (the model only: for the false-alarm tests, and to show what the push is for)"""

    def __init__(self, samprate, block_len, mark=1785.0, space=1615.0, baud=100.0, warm=64, snr=64, min_p=1 << 16, acq=2, lose=3,
                 input_scale=32767.0, max_events=64, table=None, incs=None, tb=None, start=0, gate=True, nudge=True):
        incs = (dsc_inc(mark, samprate), dsc_inc(space, samprate)) if incs is None else incs   # mark, then space
        super().__init__(samprate, block_len, incs, table, bit_length(samprate, block_len, baud) if tb is None else tb, input_scale,
                         max_events, start, widest=("P",))
        self.warm, self.snr, self.min_p, self.acq, self.lose = int(warm), int(snr), int(min_p), int(acq), int(lose)
        self.gate, self.nudge = gate, nudge
        self.bit = self.nbits = self.synced = self.bitpos = 0
        self.Ec = self.sig = self.nse = self.hi = self.lo = self.r = 0
        self.inverted = self.place = self.nsym = self.nres = self.holes = self.from_rx = self.run = self.ecc = self.eos = 0
        self.hole_mask = self.sync_sample = 0
        self.msg = [0] * MAX_SYMBOLS
        self.syncs = self.aborted = 0
        self.bits = []               # of every bit: (bit, open)

    def _file(self, flags, k):
        super()._file(Event(bytes(self.msg), self.nsym, flags | (INVERTED if self.inverted else 0), self.holes, self.from_rx,
                            self.hole_mask, self.sync_sample, (k + 1) * self.B, self.sig, self.nse))

    def _centre(self, best):
        Pm, Ps = self.powers()
        self.bit, self.hi, self.lo = int(Pm >= Ps), best, min(Pm, Ps)

    def _bit(self, k, Pl):
        """the header's steps 1 to 5 at a late point, frame k"""
        is_open = self._levels(Pl, self.nudge)  # 1 timing, 2 levels and gate
        self.bits.append((self.bit, is_open))
        # 3 register
        self.r = (self.r << 1 | self.bit) & M64
        self.nbits = (self.nbits + 1) & 0xFFFFFFFF
        # 4 sync
        if not self.synced:
            if not is_open:
                return
            place, inv = phasing(self.r, self.acq), 0
            if place < 0:
                place, inv = phasing(self.r ^ M64, self.acq), 1
            if place < 0:
                return
            self.synced, self.bitpos = 1, 0
            self.syncs = min(self.syncs + 1, 0xFFFFFFFF)
            self.inverted, self.place = inv, place
            self.nsym = self.nres = self.holes = self.from_rx = self.run = self.ecc = self.eos = 0
            self.hole_mask, self.sync_sample = 0, (k + 1) * self.B
            self.msg = [0] * MAX_SYMBOLS
            return
        # 5 message
        self.bitpos += 1
        if self.bitpos < 10:
            return
        self.bitpos = 0
        self.place += 1
        if not self.place & 1 or self.place < 17:
            return
        i = (self.place - 17) >> 1
        x = self.r ^ M64 if self.inverted else self.r
        dx, rx = x >> 50 & 1023, x & 1023
        got = is_symbol(dx) or is_symbol(rx)
        d = value_of(dx) if is_symbol(dx) else value_of(rx)
        if not is_symbol(dx) and is_symbol(rx):
            self.from_rx += 1
        self.msg[i] = d if got else 0xFF
        self.nsym = i + 1
        if not got:
            self.holes += 1
            self.hole_mask |= 1 << i
        if self.eos:                                                  # (a)
            self._file(CHECK if (not got or self.holes or d != self.ecc) else 0, k)
            self.synced = 0
            return
        if not got:
            self.run += 1
            if self.run >= self.lose:                                 # (c)
                if self.nres >= 8:
                    self._file(LOST | CHECK, k)
                else:
                    self.aborted = min(self.aborted + 1, 0xFFFFFFFF)
                self.synced = 0
                return
        else:
            self.run = 0
            self.nres += 1
            if i >= 1:
                self.ecc ^= d
            if d in (117, 122, 127):
                self.eos = 1
        if self.nsym == MAX_SYMBOLS:                                  # (b)
            self._file(TRUNCATED | CHECK, k)
            self.synced = 0

    def _frame(self, k):
        """one completed frame k: the window, then the header's step"""
        self._note("red", *self._close(12))
        if not self._tick():
            return
        best = max(self.powers())                                     # (the powers matter at the points only)
        self._note("sum", *self.sums)
        self._note("P", best)
        self._point(k, best, self._centre, self._bit)

    def status(self):
        """kq_dsc_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, bit=self.bit, nbits=self.nbits, synced=self.synced,
                    bitpos=self.bitpos, events=self.nevents, dropped=self.dropped, syncs=self.syncs, aborted=self.aborted,
                    reserved=0, sig=self.sig, nse=self.nse, ee=self.Ee, el=self.El, ec=self.Ec, pe=self.Pe, hi=self.hi, lo=self.lo, r=self.r,
                    sum=gm.pairs(self.sums), acc=gm.pairs(self.acc), inverted=self.inverted,
                    place=self.place, nsym=self.nsym, nres=self.nres, holes=self.holes, from_rx=self.from_rx, run=self.run,
                    ecc=self.ecc, eos=self.eos, reserved2=0, hole_mask=self.hole_mask, sync_sample=self.sync_sample,
                    msg=list(self.msg))


def noise_sigma(amp, esn0_db, Fs, baud=100.0):
    return gm.noise_sigma(amp, esn0_db, Fs, baud)
