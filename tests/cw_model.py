"""The CW (Morse) decoder of include/ka9q_hip.h (kq_cw_*) restated in numpy and Python ints, for the tests: the quantiser
of fsk_model, tone_model's cosine table, one correlator whose phase is a function of the sample index alone, and the
tracker, a step per completed frame.  The frame sums are taken in int64 (they stay below 2^42) and everything from the
shifts on in Python ints: there is no float after the quantiser.  The speed limits and the start speed become integers
(u_min, u_max, u0) before any sample is seen, by the header's formulas in double."""
import collections
import math

import numpy as np

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
RUN_MAX = 0x0FFFFFFF
Event = collections.namedtuple("Event", "code nelem unit start_sample end_sample peak")
STATUS = ("frames", "key", "run", "unit", "events", "dropped", "cand", "code", "nelem", "flags", "hi", "lo", "first", "last",
          "acc_i", "acc_q")           # kq_cw_status: what the issue's status shows, then the rest of what is carried

cos_table, cw_inc = gm.cos_table, gm.inc


def unit_limits(Fs, B, min_wpm, max_wpm):
    """u_min = floor(19.2 Fs / (B max_wpm)), u_max = ceil(19.2 Fs / (B min_wpm)), the speeds float32, in double"""
    lo = 19.2 * float(Fs) / (float(B) * float(np.float32(max_wpm)))
    hi = 19.2 * float(Fs) / (float(B) * float(np.float32(min_wpm)))
    return int(math.floor(lo)), int(math.ceil(hi))


def unit_start(Fs, B, wpm):
    """u0 = rint(19.2 Fs / (B wpm)) in double, wpm a float32"""
    return int(np.rint(19.2 * float(Fs) / (float(B) * float(np.float32(wpm)))))


def frame_sums(q, n0, inc, C):
    """I and Q of the samples q at n0, n0 + 1, ...: Python ints"""
    q = np.asarray(q, np.int64)
    n = np.arange(n0, n0 + len(q), dtype=np.uint64)
    j = (((n * np.uint64(inc)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)   # wraps mod 2^64: mod 2^32 is kept
    Ct = np.asarray(C, np.int64)
    return int((q * Ct[j]).sum()), int((q * Ct[(j - 256) & (TABLE - 1)]).sum())


class CwModel(gm.GridModel):
    """one slot.  table, inc: the bank's own (kq_cw_get_table, kq_cw_get_inc), or None for the model's; start: the sample
    at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, pitch=700.0, wpm=20.0, min_wpm=5.0, max_wpm=60.0, deb=2, warm=64, snr=256,
                 min_p=1 << 16, input_scale=32767.0, max_events=256, table=None, inc=None, start=0):
        super().__init__(samprate, block_len, (cw_inc(pitch, samprate) if inc is None else inc,), table, None, input_scale,
                         max_events, start)                        # no window: acc is the open frame's I and Q
        self.deb, self.warm, self.snr, self.min_p = int(deb), int(warm), int(snr), int(min_p)
        self.u_min, self.u_max = unit_limits(samprate, block_len, min_wpm, max_wpm)
        self.hi = self.lo = 0
        self.key = self.cand = self.run = 0
        self.u = min(max(unit_start(samprate, block_len, wpm), self.u_min), self.u_max)
        self.code, self.nelem, self.closed, self.worded = 1, 0, 1, 1
        self.first = self.last = 0
        self.P = []                  # of every completed frame
        self.widest = 0              # one bound for all of it

    I, Q = property(lambda self: self.acc[0]), property(lambda self: self.acc[1])

    def _file(self, code, nelem, start, end):
        super()._file(Event(code, nelem, self.u, start * self.B, end * self.B, self.hi))

    def _frame(self, k):
        """the header's tracker, steps 1 to 7, on frame k"""
        P = (self.I >> 15) ** 2 + (self.Q >> 15) ** 2
        self.widest = max(self.widest, abs(self.I), abs(self.Q), P)
        self.P.append(P)
        self.acc = [0, 0]
        self.frames = min(self.frames + 1, 0xFFFFFFFF)
        # 1 peak
        if P > self.hi:
            self.hi = P
        else:
            self.hi -= self.hi >> 8
        # 2 validity
        valid = self.frames >= self.warm and self.hi >= self.min_p and self.hi >= (self.lo >> 4) * self.snr
        # 3 threshold
        d = self.hi - self.lo if self.hi > self.lo else 0
        thr = self.lo + (d >> 3 if self.key else d >> 2)
        lev = int(valid and P >= thr)
        # 4 floor
        if lev == 0 or (self.key and self.run * 16 > 8 * self.u):
            self.lo += (P - self.lo) >> 5
        # 5 debounce
        if lev == self.key:
            self.run = min(self.run + 1 + self.cand, RUN_MAX)
            self.cand = 0
        else:
            self.cand += 1
            if self.cand >= self.deb:
                if self.key:
                    self._mark(self.run)
                    self.last = k + 1 - self.cand
                elif self.nelem == 0:
                    self.first = k + 1 - self.cand
                self.key, self.run, self.cand = lev, self.cand, 0
        # 7 space
        if not self.key:
            if not self.closed and 16 * self.run >= 2 * self.u:
                self._file(self.code, self.nelem, self.first, self.last)
                self.code, self.nelem, self.closed = 1, 0, 1
            if not self.worded and 16 * self.run >= 5 * self.u:
                self._file(1, 0, self.last, k + 1)
                self.worded = 1

    def _mark(self, run):
        """6: a mark of `run` frames closes"""
        m, u = 16 * run, self.u
        if m > 8 * u:
            self.code = 0
        elif m < 2 * u:
            self.code = 2 * self.code
            u += (m - u) >> 2
        else:
            self.code = 2 * self.code + (1 if self.code else 0)
            u += (m // 3 - u) >> 2
        self.u = min(max(u, self.u_min), self.u_max)
        self.nelem += 1
        if self.nelem > 8:
            self.code = 0
        self.closed = self.worded = 0

    def status(self):
        """kq_cw_status: every counter, the whole tracker state and the open frame's sums"""
        return dict(frames=self.frames, key=self.key, run=self.run, unit=self.u, events=self.nevents, dropped=self.dropped,
                    cand=self.cand, code=self.code, nelem=self.nelem, flags=self.closed | self.worded << 1, hi=self.hi,
                    lo=self.lo, first=self.first, last=self.last, acc_i=self.I, acc_q=self.Q)


def noise_sigma(amp, snr_db, B):
    """white noise whose power in Fs / B lies snr_db below a tone of amplitude amp: sigma^2 = amp^2 / 2 / 10^(dB / 10) B / 2"""
    return math.sqrt(amp * amp / 2.0 / 10.0 ** (snr_db / 10.0) * B / 2.0)
