"""The RTTY decoder of include/ka9q_hip.h (kq_rtty_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, two correlators whose phases are functions of the sample index alone, a sliding
window one bit long over the frames' reduced sums, and the start-stop framer, a step per completed frame.  The frame sums
are taken in int64 (they stay below 2^38) and everything from the shifts on in Python ints: there is no float after the
quantiser.  The bit length becomes an integer (tb) before any sample is seen, by the header's formula in double.  Every
intermediate is recorded in `widest`, by kind, so that a test can hold each inside the bound the header states."""
import collections
import math

import numpy as np

import fsk_model as fm
import tone_model as tm

TABLE = tm.TABLE
WAIT, IDLE, CHAR = 0, 1, 2
Event = collections.namedtuple("Event", "code flags start_sample sig nse")
STATUS = ("frames", "state", "bit", "code", "t", "events", "dropped", "ferr", "false_starts", "reserved", "sig", "nse", "start",
          "sum_im", "sum_qm", "sum_is", "sum_qs", "acc_im", "acc_qm", "acc_is", "acc_qs")

cos_table = tm.cos_table


def rtty_inc(f, Fs):
    """inc = rint(f 2^32 / Fs) in double, f a float32"""
    return int(np.rint(float(np.float32(f)) * 4294967296.0 / float(Fs)))


def bit_length(Fs, B, baud):
    """tb = rint(256 Fs / (B baud)) in double, baud a float32: the bit in 1/256 frame"""
    return int(np.rint(256.0 * float(Fs) / (float(B) * float(np.float32(baud)))))


def window(tb):
    """W = (tb + 128) >> 8 frames"""
    return (tb + 128) >> 8


class RttyModel:
    """one slot.  table, incs, tb: the bank's own (kq_rtty_get_table, kq_rtty_get_slot), or None for the model's; start:
    the sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, mark=2125.0, space=2295.0, baud=45.45, nbits=5, warm=64, snr=96, min_p=1 << 16,
                 input_scale=32767.0, max_events=256, table=None, incs=None, tb=None, start=0):
        self.Fs, self.B = float(samprate), int(block_len)
        self.nbits, self.warm, self.snr, self.min_p = int(nbits), int(warm), int(snr), int(min_p)
        self.scale, self.max_events = input_scale, max_events
        self.C = cos_table() if table is None else np.asarray(table, np.int16)
        self.incs = (rtty_inc(mark, samprate), rtty_inc(space, samprate)) if incs is None else tuple(int(v) for v in incs)
        self.tb = bit_length(samprate, block_len, baud) if tb is None else int(tb)
        self.W = window(self.tb)
        self.n = int(start)
        self.acc = [0, 0, 0, 0]                                     # I, Q of mark, I, Q of space: the open frame
        self.hist = collections.deque([(0, 0, 0, 0)] * self.W, self.W)   # the last W frames' a, b
        self.sums = [0, 0, 0, 0]
        self.sig = self.nse = 0
        self.state, self.bit, self.code, self.t, self.start = WAIT, 0, 0, 0, 0
        self.frames = self.nevents = self.dropped = self.ferr = self.false_starts = 0
        self.events = []
        self.levels = []             # of every completed frame
        self.widest = dict(acc=0, red=0, sum=0, P=0, lvl=0, prod=0)

    def _file(self, flags):
        self.nevents = min(self.nevents + 1, 0xFFFFFFFF)
        if len(self.events) >= self.max_events:
            self.dropped = min(self.dropped + 1, 0xFFFFFFFF)
        else:
            self.events.append(Event(self.code, flags, self.start * self.B, self.sig, self.nse))

    def _frame(self, k):
        """the header's steps 1 to 4 on frame k, behind the window"""
        wd = self.widest
        red = tuple(v >> 12 for v in self.acc)
        wd["acc"] = max(wd["acc"], *(abs(v) for v in self.acc))
        wd["red"] = max(wd["red"], *(abs(v) for v in red))
        self.acc = [0, 0, 0, 0]
        old = self.hist[0]
        self.hist.append(red)
        self.sums = [s + a - o for s, a, o in zip(self.sums, red, old)]
        Pm = self.sums[0] ** 2 + self.sums[1] ** 2
        Ps = self.sums[2] ** 2 + self.sums[3] ** 2
        wd["sum"] = max(wd["sum"], *(abs(v) for v in self.sums))
        wd["P"] = max(wd["P"], Pm, Ps)
        # 1 count and level
        self.frames = min(self.frames + 1, 0xFFFFFFFF)
        hi, lo, lev = max(Pm, Ps), min(Pm, Ps), int(Pm >= Ps)
        self.levels.append(lev)
        # 2 levels
        samp = self.state == CHAR and self.t - 256 < 128
        if self.state != CHAR or samp:
            sh = 4 if samp else 6
            self.sig += (hi - self.sig) >> sh
            self.nse += (lo - self.nse) >> sh
            wd["lvl"] = max(wd["lvl"], self.sig, self.nse)
        # 3 validity
        wd["prod"] = max(wd["prod"], 16 * self.sig, self.nse * self.snr)
        if not (self.frames >= self.warm and self.sig >= self.min_p and 16 * self.sig >= self.nse * self.snr):
            self.state = WAIT
            return
        # 4 framer
        if self.state == WAIT:
            if lev:
                self.state = IDLE
        elif self.state == IDLE:
            if not lev:
                self.state, self.t, self.bit, self.code, self.start = CHAR, self.tb >> 1, -1, 0, k
        else:
            self.t -= 256
            if not samp:
                return
            self.t += self.tb
            if self.bit < 0:
                if lev:
                    self.false_starts = min(self.false_starts + 1, 0xFFFFFFFF)
                    self.state = IDLE
                else:
                    self.bit = 0
            elif self.bit < self.nbits:
                self.code |= lev << self.bit
                self.bit += 1
            elif lev:
                self._file(0)
                self.state = IDLE
            else:
                self._file(1)
                self.ferr = min(self.ferr + 1, 0xFFFFFFFF)
                self.state = WAIT

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
        """kq_rtty_status: every counter, the framer and level state, the window sums and the open frame's sums"""
        return dict(frames=self.frames, state=self.state, bit=self.bit, code=self.code, t=self.t, events=self.nevents,
                    dropped=self.dropped, ferr=self.ferr, false_starts=self.false_starts, reserved=0, sig=self.sig,
                    nse=self.nse, start=self.start, sum_im=self.sums[0], sum_qm=self.sums[1], sum_is=self.sums[2],
                    sum_qs=self.sums[3], acc_im=self.acc[0], acc_qm=self.acc[1], acc_is=self.acc[2], acc_qs=self.acc[3])

    def clear_events(self):
        self.events = []


def noise_sigma(amp, ebn0_db, Fs, baud):
    """white noise that leaves a tone of amplitude amp at Eb/N0: sigma^2 = (amp^2 / 2) / 10^(dB / 10) Fs / (2 baud)"""
    return math.sqrt(amp * amp / 2.0 / 10.0 ** (ebn0_db / 10.0) * float(Fs) / (2.0 * float(baud)))
