"""The ALE decoder of include/ka9q_hip.h (kq_ale_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, eight correlators whose phase is a function of the sample index alone, a sliding
window one symbol long over the frames' reduced sums, the largest of the eight powers, the early / centre / late clock on
it, the levels and the gate, the 147-bit register, and the word attempt: majority vote, de-interleave, Golay (24,12) by
the two 4096-entry tables of ka9q_sdr_amd/ale2g.py, word sync.  The frame sums are taken in int64 (they stay below 2^38)
and everything from the shifts on in Python ints: there is no float after the quantiser.  The symbol length becomes an
integer (tb) before any sample is seen, by the header's formula in double."""
import collections

import numpy as np

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm
from ka9q_sdr_amd import ale2g

TABLE = gm.TABLE
NT = 8
M49 = (1 << 49) - 1
Event = collections.namedtuple("Event", "word flags err_a err_b split reserved end_sample sig nse")
STATUS = ("frames", "ph", "t", "sym", "nsym", "sync_at", "wpos", "synced", "bad", "events", "dropped", "reserved", "sig", "nse",
          "ee", "el", "pe", "pc", "oth", "r0", "r1", "r2", "sum", "acc")
PARITY = [int(v) for v in ale2g.PARITY]
ERRORS = [int(v) for v in ale2g.ERRORS]
IN_SET = [chr(c) in ale2g.CHARSET for c in range(128)]

cos_table, symbol_length, window = gm.cos_table, gm.period, gm.window


def ale_inc(f0, df, Fs):
    """inc[t] = rint((f0 + t df) 2^32 / Fs) in double, f0 and df floats, the tone's frequency a double"""
    f0, df = float(np.float32(f0)), float(np.float32(df))
    return [int(np.rint((f0 + t * df) * 4294967296.0 / float(Fs))) for t in range(NT)]


def even_bits(x):
    """bits 0, 2, 4 .. 46 of x, packed"""
    return sum((x >> (2 * i) & 1) << i for i in range(24))


def attempt(r0, r1, r2):
    """the header's vote, de-interleave and Golay: (word, err_a, err_b, split, stuff), word from the corrected halves, or
    from the data bits as they are where a half's err is 4"""
    maj = (r0 & r1) | (r0 & r2) | (r1 & r2)
    split = bin((r0 ^ r1) | (r0 ^ r2)).count("1")
    e = maj >> 1
    A, Bh = even_bits(e >> 1), even_bits(e) ^ 0xFFF
    ea, eb = ERRORS[PARITY[A >> 12] ^ (A & 0xFFF)], ERRORS[PARITY[Bh >> 12] ^ (Bh & 0xFFF)]
    return ((A >> 12) ^ (ea & 0xFFF)) << 12 | (Bh >> 12) ^ (eb & 0xFFF), ea >> 12, eb >> 12, split, maj & 1


def address_like(w):
    """every preamble but CMD takes its three characters from the 38-set"""
    return w >> 21 == ale2g.CMD or (IN_SET[w >> 14 & 0x7F] and IN_SET[w >> 7 & 0x7F] and IN_SET[w & 0x7F])


class AleModel(gm.GridModel):
    """one slot.  table, inc, tb: the bank's own (kq_ale_get_table, kq_ale_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it).  gate=False leaves the validity gate open (the model only: for the
    false-alarm tests)"""

    def __init__(self, samprate, block_len, f0=750.0, df=250.0, baud=125.0, warm=64, snr=80, min_p=1 << 16, acq_err=1, lose=2,
                 input_scale=32767.0, max_events=256, table=None, inc=None, tb=None, start=0, gate=True):
        super().__init__(samprate, block_len, ale_inc(f0, df, samprate) if inc is None else inc, table,
                         symbol_length(samprate, block_len, baud) if tb is None else tb, input_scale, max_events, start,
                         widest=("P", "oth"))
        self.warm, self.snr, self.min_p, self.acq_err, self.lose = int(warm), int(snr), int(min_p), int(acq_err), int(lose)
        self.gate = gate
        self.sym = 0
        self.sig = self.nse = self.Pc = self.oth = 0
        self.r = [0, 0, 0]
        self.nsym = self.sync_at = self.wpos = self.synced = self.bad = 0
        self.syms = []               # of every symbol: (tone, valid)

    def _file(self, word, flags, ea, eb, split, k):
        super()._file(Event(word, flags, ea, eb, split, 0, (k + 1) * self.B, self.sig, self.nse))

    def _centre(self, best):
        P = self.powers()
        self.sym = P.index(best)                                        # ties to the lowest tone
        self.Pc = best
        self.oth = sum(p >> 3 for t, p in enumerate(P) if t != self.sym)
        self._note("oth", self.oth)

    def _symbol(self, k, Pl):
        """the header's steps 1 to 5 at a late point, frame k"""
        # 1 timing
        self._timing(Pl)
        # 2 levels and gate
        self.sig += (self.Pc - self.sig) >> 4
        self.nse += (self.oth - self.nse) >> 4
        valid = self.frames >= self.warm and self.sig >= self.min_p and 16 * self.sig >= self.snr * self.nse
        valid = valid or not self.gate
        self.syms.append((self.sym, valid))
        # 3 register
        g = ale2g.GRAY[self.sym]
        r0, r1, r2 = self.r
        self.r = [(r0 << 3 | r1 >> 46) & M49, (r1 << 3 | r2 >> 46) & M49, (r2 << 3 | g) & M49]
        self.nsym = (self.nsym + 1) & 0xFFFFFFFF
        if self.synced:
            self.wpos += 1
        # 4 gate
        if not valid:
            self.synced = self.bad = self.wpos = 0
            return
        # 5 word attempt
        if self.synced and self.wpos < 49:
            return
        word, ea, eb, split, stuff = attempt(*self.r)
        if not self.synced:
            if ea <= self.acq_err and eb <= self.acq_err and stuff == 0 and address_like(word):
                self.synced, self.sync_at, self.wpos, self.bad = 1, self.nsym, 0, 0
                self._file(word, 0, ea, eb, split, k)
            return
        self.wpos = 0
        if ea < 4 and eb < 4:
            self.bad = 0
            self._file(word, 0, ea, eb, split, k)
        else:
            self._file(word, 1, ea, eb, split, k)
            self.bad += 1
            if self.bad >= self.lose:
                self.synced = self.bad = 0

    def _frame(self, k):
        """one completed frame k: the window, then the header's step"""
        red = self._close(12)
        if not self._tick():
            return
        best = max(self.powers())                                       # (the powers matter at the points only)
        self._note("red", *red)
        self._note("sum", *self.sums)
        self._note("P", best)
        self._point(k, best, self._centre, self._symbol)

    def status(self):
        """kq_ale_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, sym=self.sym, nsym=self.nsym, sync_at=self.sync_at, wpos=self.wpos,
                    synced=self.synced, bad=self.bad, events=self.nevents, dropped=self.dropped, reserved=0, sig=self.sig,
                    nse=self.nse, ee=self.Ee, el=self.El, pe=self.Pe, pc=self.Pc, oth=self.oth, r0=self.r[0], r1=self.r[1],
                    r2=self.r[2], sum=gm.pairs(self.sums), acc=gm.pairs(self.acc))


def noise_sigma(amp, esn0_db, Fs, baud=125.0):
    return gm.noise_sigma(amp, esn0_db, Fs, baud)
