"""The PSK decoder of include/ka9q_hip.h (kq_psk_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, one correlator whose phase is a function of the sample index alone, a sliding window
one symbol long over the frames' reduced sums, and the symbol clock, the differential detector, the rotation estimate and
the Varicode shift register, a step per completed frame.  The frame sums are taken in int64 (they stay below 2^38) and
everything from the shifts on in Python ints: there is no float after the quantiser.  The symbol length becomes an integer
(tb) before any sample is seen, by the header's formula in double.  Every intermediate is recorded in `widest`, by kind, so
that a test can hold each inside the bound the header states."""
import collections
import math

import numpy as np

import fsk_model as fm
import tone_model as tm

TABLE = tm.TABLE
Event = collections.namedtuple("Event", "code flags end_sample sig rot_r rot_i")
STATUS = ("frames", "ph", "t", "shreg", "over", "events", "dropped", "reserved", "sig", "qre", "qim", "ee", "el", "pe", "pc",
          "rot_r", "rot_i", "cr", "ci", "pr", "pi", "sum_i", "sum_q", "acc_i", "acc_q")

cos_table = tm.cos_table


def psk_inc(f, Fs):
    """inc = rint(f 2^32 / Fs) in double, f a float32"""
    return int(np.rint(float(np.float32(f)) * 4294967296.0 / float(Fs)))


def symbol_length(Fs, B, baud):
    """tb = rint(256 Fs / (B baud)) in double, baud a float32: the symbol in 1/256 frame"""
    return int(np.rint(256.0 * float(Fs) / (float(B) * float(np.float32(baud)))))


def window(tb):
    """W = (tb + 128) >> 8 frames"""
    return (tb + 128) >> 8


def norm(x, y):
    """both shifted down until the larger magnitude is below 2^24"""
    s = max(max(abs(x), abs(y)).bit_length() - 24, 0)
    return x >> s, y >> s


class PskModel:
    """one slot.  table, inc, tb: the bank's own (kq_psk_get_table, kq_psk_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, pitch=1000.0, baud=31.25, warm=64, snr=32, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, table=None, inc=None, tb=None, start=0):
        self.Fs, self.B = float(samprate), int(block_len)
        self.warm, self.snr, self.min_p = int(warm), int(snr), int(min_p)
        self.scale, self.max_events = input_scale, max_events
        self.C = cos_table() if table is None else np.asarray(table, np.int16)
        self.inc = psk_inc(pitch, samprate) if inc is None else int(inc)
        self.tb = symbol_length(samprate, block_len, baud) if tb is None else int(tb)
        self.W = window(self.tb)
        self.q = self.tb >> 2
        self.n = int(start)
        self.acc = [0, 0]                                           # I, Q of the open frame
        self.hist = collections.deque([(0, 0)] * self.W, self.W)    # the last W frames' a, b
        self.sums = [0, 0]
        self.ph = self.t = self.shreg = self.over = 0
        self.sig = self.qre = self.qim = self.Ee = self.El = self.Pe = self.Pc = 0
        self.R, self.c, self.p = [0, 0], (0, 0), (0, 0)
        self.frames = self.nevents = self.dropped = 0
        self.events = []
        self.bits = []               # of every symbol: (bit, valid)
        self.widest = dict(acc=0, red=0, sum=0, P=0, D=0, R=0, n=0, dec=0, lvl=0, prod=0)

    def _file(self, code, flags, k, r):
        self.nevents = min(self.nevents + 1, 0xFFFFFFFF)
        if len(self.events) >= self.max_events:
            self.dropped = min(self.dropped + 1, 0xFFFFFFFF)
        else:
            self.events.append(Event(code, flags, (k + 1) * self.B, self.sig, r[0], r[1]))

    def _symbol(self, k, Pl):
        """the header's steps 1 to 8 at a late point, frame k"""
        wd, tb = self.widest, self.tb
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
        # 2 product
        (cr, ci), (pr, pi) = self.c, self.p
        D = (cr * pr + ci * pi, ci * pr - cr * pi)
        self.p = self.c
        # 3 normalise
        d = norm(*D)
        r = norm(*self.R) if self.R != [0, 0] else (1, 0)
        # 4 decision
        Re, Im = d[0] * r[0] + d[1] * r[1], d[1] * r[0] - d[0] * r[1]
        bit = int(Re >= 0)
        # 5 rotation
        Dp = D if bit else (-D[0], -D[1])
        self.R = [self.R[0] + ((Dp[0] - self.R[0]) >> 4), self.R[1] + ((Dp[1] - self.R[1]) >> 4)]
        if 2 * self.R[0] < abs(self.R[1]):
            self.R[0] = abs(self.R[1]) >> 1
        # 6 levels
        self.qre += (abs(Re) - self.qre) >> 4
        self.qim += (abs(Im) - self.qim) >> 4
        self.sig += (self.Pc - self.sig) >> 4
        wd["D"] = max(wd["D"], abs(D[0]), abs(D[1]))
        wd["R"] = max(wd["R"], abs(self.R[0]), abs(self.R[1]))
        wd["n"] = max(wd["n"], *(abs(v) for v in d + r))
        wd["dec"] = max(wd["dec"], abs(Re), abs(Im))
        wd["lvl"] = max(wd["lvl"], self.sig, self.Ee, self.El)
        wd["prod"] = max(wd["prod"], 16 * self.qre, self.snr * self.qim)
        # 7 validity
        valid = self.frames >= self.warm and self.sig >= self.min_p and 16 * self.qre >= self.snr * self.qim
        self.bits.append((bit, valid))
        if not valid:
            self.shreg = self.over = 0
            return
        # 8 Varicode
        if self.shreg & 0x2000:
            self.over = 1
        self.shreg = (self.shreg << 1 | bit) & 0x3FFF
        if (self.shreg & 3) == 0:
            code = self.shreg >> 2
            if code:
                self._file(code, 1 if code > 1023 else self.over, k, r)
            self.shreg = self.over = 0

    def _frame(self, k):
        """one completed frame k: the window, then the header's step"""
        wd = self.widest
        red = tuple(v >> 13 for v in self.acc)
        wd["acc"] = max(wd["acc"], *(abs(v) for v in self.acc))
        wd["red"] = max(wd["red"], *(abs(v) for v in red))
        self.acc = [0, 0]
        old = self.hist[0]
        self.hist.append(red)
        self.sums = [s + a - o for s, a, o in zip(self.sums, red, old)]
        P = self.sums[0] ** 2 + self.sums[1] ** 2
        wd["sum"] = max(wd["sum"], *(abs(v) for v in self.sums))
        wd["P"] = max(wd["P"], P)
        self.frames = min(self.frames + 1, 0xFFFFFFFF)
        self.t -= 256
        if self.t >= 128:
            return
        if self.ph == 0:
            self.Pe = P
            self.t += self.q
            self.ph = 1
        elif self.ph == 1:
            self.c = (self.sums[0], self.sums[1])
            self.Pc = P
            self.t += self.q
            self.ph = 2
        else:
            self.ph = 0
            self._symbol(k, P)

    def feed(self, x, s16=False):
        q = fm.quantise(x, self.scale, s16)
        if not len(q):
            return self
        B, n0 = self.B, self.n
        n = np.arange(n0, n0 + len(q), dtype=np.uint64)
        Ct = self.C.astype(np.int64)
        cuts = np.concatenate([[0], np.arange(B - n0 % B, len(q), B)]).astype(np.int64)     # where the chunk's frames begin
        ends = np.concatenate([cuts[1:], [len(q)]])
        j = (((n * np.uint64(self.inc)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)   # mod 2^64 keeps mod 2^32
        part = [np.add.reduceat(q * Ct[j], cuts).tolist(),                                   # exact: int64, below 2^38
                np.add.reduceat(q * Ct[(j - 256) & (TABLE - 1)], cuts).tolist()]
        for i, e in enumerate(ends.tolist()):
            self.acc[0] += part[0][i]
            self.acc[1] += part[1][i]
            self.n = n0 + e
            if self.n % B == 0:
                self._frame(self.n // B - 1)
        return self

    def status(self):
        """kq_psk_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, shreg=self.shreg, over=self.over, events=self.nevents,
                    dropped=self.dropped, reserved=0, sig=self.sig, qre=self.qre, qim=self.qim, ee=self.Ee, el=self.El,
                    pe=self.Pe, pc=self.Pc, rot_r=self.R[0], rot_i=self.R[1], cr=self.c[0], ci=self.c[1], pr=self.p[0], pi=self.p[1],
                    sum_i=self.sums[0], sum_q=self.sums[1], acc_i=self.acc[0], acc_q=self.acc[1])

    def clear_events(self):
        self.events = []


def noise_sigma(amp, esn0_db, Fs, baud):
    """white noise that leaves a carrier of amplitude amp at Es/N0, the symbol's energy taken at the carrier's level:
    sigma^2 = (amp^2 / 2) / 10^(dB / 10) Fs / (2 baud)"""
    return math.sqrt(amp * amp / 2.0 / 10.0 ** (esn0_db / 10.0) * float(Fs) / (2.0 * float(baud)))
