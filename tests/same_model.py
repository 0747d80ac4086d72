"""The EAS / SAME decoder of include/ka9q_hip.h (kq_same_*) restated in numpy and Python ints, for the tests, from the
header's text: grid_model's front half and clock (kq_dsc_*'s: the quantiser, the cosine table, two correlators whose phases
are functions of the sample index alone, the window one bit long, the early / centre / late clock with its push from half
a bit out, the levels and the gate), then the 64-bit register, the attempt on the two 48-bit patterns, and in sync a byte at
every eighth bit with the three ways a burst ends.  Everything from the shifts on is Python ints: there is no float after
the quantiser."""
import collections

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
M64 = (1 << 64) - 1
M48 = (1 << 48) - 1
M32 = 0xFFFFFFFF
START, BAD, END = 1, 2, 4
COMPLETE, LOST, LENGTH = 1, 2, 3
MARK, SPACE, BAUD = 6250.0 / 3.0, 1562.5, 3125.0 / 6.0
Event = collections.namedtuple("Event", "code flags index errs end_sample sig nse")
STATUS = ("frames", "ph", "t", "bit", "synced", "bitpos", "nbytes", "bad_run", "plus", "dashes", "events", "dropped", "syncs",
          "eoms", "complete", "lost", "truncated", "sync_sample", "sig", "nse", "ee", "el", "ec", "pe", "hi", "lo", "r", "sum", "acc")

cos_table, same_inc, bit_length, window = gm.cos_table, gm.inc, gm.period, gm.window


def rev8(b):
    return int("{:08b}".format(b & 255)[::-1], 2)


def pattern(data):
    """48 bits of six bytes in sending order, the first sent highest, each byte turned end for end"""
    v = 0
    for b in data:
        v = v << 8 | rev8(b)
    return v


PH, PE = pattern(b"\xab\xabZCZC"), pattern(b"\xab\xabNNNN")


class SameModel(gm.GridModel):
    """one slot.  table, incs, tb: the bank's own (kq_same_get_table, kq_same_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it).  gate=False leaves the gate open (the model only)"""

    def __init__(self, samprate, block_len, mark=MARK, space=SPACE, baud=BAUD, warm=64, snr=64, min_p=1 << 16, sync_errs=2,
                 lose=3, max_len=248, input_scale=32767.0, max_events=1024, table=None, incs=None, tb=None, start=0, gate=True):
        incs = (same_inc(mark, samprate), same_inc(space, samprate)) if incs is None else incs   # mark, then space
        super().__init__(samprate, block_len, incs, table, bit_length(samprate, block_len, baud) if tb is None else tb, input_scale,
                         max_events, start, widest=("P",))
        self.warm, self.snr, self.min_p = int(warm), int(snr), int(min_p)
        self.sync_errs, self.lose, self.max_len, self.gate = int(sync_errs), int(lose), int(max_len), gate
        self.bit = self.synced = self.bitpos = self.nbytes = self.bad_run = self.plus = self.dashes = 0
        self.Ec = self.sig = self.nse = self.hi = self.lo = self.r = self.sync_sample = 0
        self.syncs = self.eoms = self.complete = self.lost = self.truncated = 0
        self.bits = []               # of every bit: (bit, open)

    def _centre(self, best):
        Pm, Ps = self.powers()
        self.bit, self.hi, self.lo = int(Pm >= Ps), best, min(Pm, Ps)

    def _ev(self, k, code, flags, index=0, errs=0):
        self._file(Event(code, flags, index, errs, (k + 1) * self.B, self.sig, self.nse))

    def _bit(self, k, Pl):
        """the header's steps 1 to 5 at a late point, frame k"""
        is_open = self._levels(Pl)  # 1 timing, 2 levels and gate
        self.bits.append((self.bit, is_open))
        # 3 register
        self.r = (self.r << 1 | self.bit) & M64
        # 4 sync
        if not self.synced:
            if not is_open:
                return
            dh, de = bin((self.r ^ PH) & M48).count("1"), bin((self.r ^ PE) & M48).count("1")
            if dh <= self.sync_errs:
                self.synced, self.bitpos, self.nbytes, self.bad_run, self.plus, self.dashes = 1, 0, 0, 0, 0, 0
                self.syncs = min(self.syncs + 1, M32)
                self.sync_sample = (k + 1) * self.B
                self._ev(k, ord("Z"), START, 0, dh)
            elif de <= self.sync_errs:
                self.eoms = min(self.eoms + 1, M32)
                self.sync_sample = (k + 1) * self.B
                self._ev(k, ord("N"), START, 0, de)
            return
        # 5 text
        self.bitpos += 1
        if self.bitpos < 8:
            return
        self.bitpos = 0
        b = rev8(self.r)
        if 0x20 <= b <= 0x7E:
            self._ev(k, b, 0, self.nbytes)
            self.bad_run = 0
            if b == ord("+"):
                self.plus = 1
            elif b == ord("-") and self.plus:
                self.dashes += 1
        else:
            self._ev(k, b, BAD, self.nbytes)
            self.bad_run += 1
        self.nbytes += 1
        if self.dashes == 3:
            why, self.complete = COMPLETE, min(self.complete + 1, M32)
        elif self.bad_run == self.lose:
            why, self.lost = LOST, min(self.lost + 1, M32)
        elif self.nbytes == self.max_len:
            why, self.truncated = LENGTH, min(self.truncated + 1, M32)
        else:
            return
        self._ev(k, why, END, self.nbytes)
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
        """kq_same_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, bit=self.bit, synced=self.synced, bitpos=self.bitpos,
                    nbytes=self.nbytes, bad_run=self.bad_run, plus=self.plus, dashes=self.dashes, events=self.nevents,
                    dropped=self.dropped, syncs=self.syncs, eoms=self.eoms, complete=self.complete, lost=self.lost,
                    truncated=self.truncated, sync_sample=self.sync_sample, sig=self.sig, nse=self.nse, ee=self.Ee, el=self.El,
                    ec=self.Ec, pe=self.Pe, hi=self.hi, lo=self.lo, r=self.r, sum=gm.pairs(self.sums), acc=gm.pairs(self.acc))


def noise_sigma(amp, esn0_db, Fs, baud=BAUD):
    return gm.noise_sigma(amp, esn0_db, Fs, baud)
