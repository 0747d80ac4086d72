"""The DSC decoder of include/ka9q_hip.h (kq_dsc_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, two correlators whose phases are functions of the sample index alone, a sliding window
one bit long over the frames' reduced sums (rtty_model's front half), the early / centre / late clock on the larger of
the two powers with its push from half a bit out, the levels and the gate, the 64-bit register, the attempt on the phasing sequence, and the message resolved
from its DX and RX copies up to its end.  The frame sums are taken in int64 (they stay below 2^38) and everything from the
shifts on in Python ints: there is no float after the quantiser.  The bit length becomes an integer (tb) before any sample
is seen, by the header's formula in double."""
import collections
import math

import numpy as np

import fsk_model as fm
import tone_model as tm

TABLE = tm.TABLE
M64 = (1 << 64) - 1
MAX_SYMBOLS = 64
W125 = 0b1011111001
CHECK, TRUNCATED, LOST, INVERTED = 1, 2, 4, 8
Event = collections.namedtuple("Event", "sym nsym flags holes from_rx hole_mask sync_sample end_sample sig nse")
STATUS = ("frames", "ph", "t", "bit", "nbits", "synced", "bitpos", "events", "dropped", "syncs", "aborted", "reserved", "sig",
          "nse", "ee", "el", "ec", "pe", "hi", "lo", "r", "sum", "acc", "inverted", "place", "nsym", "nres", "holes", "from_rx", "run",
          "ecc", "eos", "reserved2", "hole_mask", "sync_sample", "msg")

cos_table = tm.cos_table


def dsc_inc(f, Fs):
    """inc = rint(f 2^32 / Fs) in double, f a float32"""
    return int(np.rint(float(np.float32(f)) * 4294967296.0 / float(Fs)))


def bit_length(Fs, B, baud):
    """tb = rint(256 Fs / (B baud)) in double, baud a float32: the bit in 1/256 frame"""
    return int(np.rint(256.0 * float(Fs) / (float(B) * float(np.float32(baud)))))


def window(tb):
    """W = (tb + 128) >> 8 frames"""
    return (tb + 128) >> 8


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


class DscModel:
    """one slot.  table, incs, tb: the bank's own (kq_dsc_get_table, kq_dsc_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it).  gate=False leaves the gate open, nudge=False leaves out step 1's push from half a bit
    out (the model only: for the false-alarm tests, and to show what the push is for)"""

    def __init__(self, samprate, block_len, mark=1785.0, space=1615.0, baud=100.0, warm=64, snr=64, min_p=1 << 16, acq=2, lose=3,
                 input_scale=32767.0, max_events=64, table=None, incs=None, tb=None, start=0, gate=True, nudge=True):
        self.Fs, self.B = float(samprate), int(block_len)
        self.warm, self.snr, self.min_p, self.acq, self.lose = int(warm), int(snr), int(min_p), int(acq), int(lose)
        self.scale, self.max_events, self.gate, self.nudge = input_scale, max_events, gate, nudge
        self.C = cos_table() if table is None else np.asarray(table, np.int16)
        self.incs = (dsc_inc(mark, samprate), dsc_inc(space, samprate)) if incs is None else tuple(int(v) for v in incs)
        self.tb = bit_length(samprate, block_len, baud) if tb is None else int(tb)
        self.W = window(self.tb)
        self.q = self.tb >> 2
        self.n = int(start)
        self.acc = [0, 0, 0, 0]                                     # I, Q of mark, I, Q of space: the open frame
        self.hist = collections.deque([(0, 0, 0, 0)] * self.W, self.W)
        self.sums = [0, 0, 0, 0]
        self.ph = self.t = self.bit = self.nbits = self.synced = self.bitpos = 0
        self.Ec = self.sig = self.nse = self.Ee = self.El = self.Pe = self.hi = self.lo = self.r = 0
        self.inverted = self.place = self.nsym = self.nres = self.holes = self.from_rx = self.run = self.ecc = self.eos = 0
        self.hole_mask = self.sync_sample = 0
        self.msg = [0] * MAX_SYMBOLS
        self.frames = self.nevents = self.dropped = self.syncs = self.aborted = 0
        self.events = []
        self.bits = []               # of every bit: (bit, open)
        self.widest = dict(acc=0, red=0, sum=0, P=0)

    def _file(self, flags, k):
        self.nevents = min(self.nevents + 1, 0xFFFFFFFF)
        if len(self.events) >= self.max_events:
            self.dropped = min(self.dropped + 1, 0xFFFFFFFF)
        else:
            self.events.append(Event(bytes(self.msg), self.nsym, flags | (INVERTED if self.inverted else 0), self.holes,
                                     self.from_rx, self.hole_mask, self.sync_sample, (k + 1) * self.B, self.sig, self.nse))

    def _bit(self, k, Pl):
        """the header's steps 1 to 5 at a late point, frame k"""
        tb = self.tb
        # 1 timing
        self.Ee += (self.Pe - self.Ee) >> 3
        self.El += (Pl - self.El) >> 3
        m = max(self.Ee, self.El)
        adj = 0
        if self.Ee > self.El and self.Ee - self.El > (m >> 3):
            adj = -(tb >> 5)
        elif self.El > self.Ee and self.El - self.Ee > (m >> 3):
            adj = tb >> 5
        self.t += tb - 2 * self.q + adj
        self.Ec += (self.hi - self.Ec) >> 3
        if self.nudge and adj == 0 and self.Ec + (m >> 3) < min(self.Ee, self.El):
            self.t += tb >> 5                                        # half a bit out: the walk has no slope there
        # 2 levels and gate
        self.sig += (self.hi - self.sig) >> 4
        self.nse += (self.lo - self.nse) >> 4
        is_open = self.frames >= self.warm and self.sig >= self.min_p and 16 * self.sig >= self.snr * self.nse
        is_open = is_open or not self.gate
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
        wd = self.widest
        red = tuple(v >> 12 for v in self.acc)
        wd["acc"] = max(wd["acc"], *(abs(v) for v in self.acc))
        wd["red"] = max(wd["red"], *(abs(v) for v in red))
        self.acc = [0, 0, 0, 0]
        old = self.hist[0]
        self.hist.append(red)
        self.sums = [s + a - o for s, a, o in zip(self.sums, red, old)]
        self.frames = min(self.frames + 1, 0xFFFFFFFF)
        self.t -= 256
        if self.t >= 128:
            return
        Pm = self.sums[0] ** 2 + self.sums[1] ** 2                    # (the powers matter at the points only)
        Ps = self.sums[2] ** 2 + self.sums[3] ** 2
        best = max(Pm, Ps)
        wd["sum"] = max(wd["sum"], *(abs(v) for v in self.sums))
        wd["P"] = max(wd["P"], best)
        if self.ph == 0:
            self.Pe = best
            self.t += self.q
            self.ph = 1
        elif self.ph == 1:
            self.bit, self.hi, self.lo = int(Pm >= Ps), best, min(Pm, Ps)
            self.t += self.q
            self.ph = 2
        else:
            self.ph = 0
            self._bit(k, best)

    def feed(self, x, s16=False):
        q = fm.quantise(x, self.scale, s16)
        if not len(q):
            return self
        B, n0 = self.B, self.n
        n = np.arange(n0, n0 + len(q), dtype=np.uint64)
        Ct = self.C.astype(np.int64)
        cuts = np.concatenate([[0], np.arange(B - n0 % B, len(q), B)]).astype(np.int64)     # where the chunk's frames begin
        ends = np.concatenate([cuts[1:], [len(q)]])
        part = []
        for inc in self.incs:
            j = (((n * np.uint64(inc)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)   # mod 2^64 keeps mod 2^32
            part.append(np.add.reduceat(q * Ct[j], cuts).tolist())                         # exact: int64, below 2^38
            part.append(np.add.reduceat(q * Ct[(j - 256) & (TABLE - 1)], cuts).tolist())
        for i, e in enumerate(ends.tolist()):
            for c in range(4):
                self.acc[c] += part[c][i]
            self.n = n0 + e
            if self.n % B == 0:
                self._frame(self.n // B - 1)
        return self

    def status(self):
        """kq_dsc_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, bit=self.bit, nbits=self.nbits, synced=self.synced,
                    bitpos=self.bitpos, events=self.nevents, dropped=self.dropped, syncs=self.syncs, aborted=self.aborted,
                    reserved=0, sig=self.sig, nse=self.nse, ee=self.Ee, el=self.El, ec=self.Ec, pe=self.Pe, hi=self.hi, lo=self.lo, r=self.r,
                    sum=[self.sums[0:2], self.sums[2:4]], acc=[self.acc[0:2], self.acc[2:4]], inverted=self.inverted,
                    place=self.place, nsym=self.nsym, nres=self.nres, holes=self.holes, from_rx=self.from_rx, run=self.run,
                    ecc=self.ecc, eos=self.eos, reserved2=0, hole_mask=self.hole_mask, sync_sample=self.sync_sample,
                    msg=list(self.msg))

    def clear_events(self):
        self.events = []


def noise_sigma(amp, esn0_db, Fs, baud=100.0):
    """white noise that leaves a tone of amplitude amp at Es/N0: sigma^2 = (amp^2 / 2) / 10^(dB / 10) Fs / (2 baud)"""
    return math.sqrt(amp * amp / 2.0 / 10.0 ** (esn0_db / 10.0) * float(Fs) / (2.0 * float(baud)))
