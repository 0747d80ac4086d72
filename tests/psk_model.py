"""The PSK decoder of include/ka9q_hip.h (kq_psk_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, one correlator whose phase is a function of the sample index alone, a sliding window
one symbol long over the frames' reduced sums, and the symbol clock, the differential detector, the rotation estimate and
the Varicode shift register, a step per completed frame.  The frame sums are taken in int64 (they stay below 2^38) and
everything from the shifts on in Python ints: there is no float after the quantiser.  The symbol length becomes an integer
(tb) before any sample is seen, by the header's formula in double.  Every intermediate is recorded in `widest`, by kind, so
that a test can hold each inside the bound the header states."""
import collections

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
Event = collections.namedtuple("Event", "code flags end_sample sig rot_r rot_i")
STATUS = ("frames", "ph", "t", "shreg", "over", "events", "dropped", "reserved", "sig", "qre", "qim", "ee", "el", "pe", "pc",
          "rot_r", "rot_i", "cr", "ci", "pr", "pi", "sum_i", "sum_q", "acc_i", "acc_q")

cos_table, psk_inc, symbol_length, window, noise_sigma = gm.cos_table, gm.inc, gm.period, gm.window, gm.noise_sigma


def norm(x, y):
    """both shifted down until the larger magnitude is below 2^24"""
    s = max(max(abs(x), abs(y)).bit_length() - 24, 0)
    return x >> s, y >> s


class PskModel(gm.GridModel):
    """one slot.  table, inc, tb: the bank's own (kq_psk_get_table, kq_psk_get_slot), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, pitch=1000.0, baud=31.25, warm=64, snr=32, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, table=None, inc=None, tb=None, start=0):
        super().__init__(samprate, block_len, (psk_inc(pitch, samprate) if inc is None else inc,), table,
                         symbol_length(samprate, block_len, baud) if tb is None else tb, input_scale, max_events, start,
                         widest=("P", "D", "R", "n", "dec", "lvl", "prod"))
        self.warm, self.snr, self.min_p = int(warm), int(snr), int(min_p)
        self.shreg = self.over = 0
        self.sig = self.qre = self.qim = self.Pc = 0
        self.R, self.c, self.p = [0, 0], (0, 0), (0, 0)
        self.bits = []               # of every symbol: (bit, valid)

    def _centre(self, P):
        self.c = (self.sums[0], self.sums[1])
        self.Pc = P

    def _symbol(self, k, Pl):
        """the header's steps 1 to 8 at a late point, frame k"""
        wd = self.widest
        # 1 timing
        self._timing(Pl)
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
                self._file(Event(code, 1 if code > 1023 else self.over, (k + 1) * self.B, self.sig, r[0], r[1]))
            self.shreg = self.over = 0

    def _frame(self, k):
        """one completed frame k: the window, then the header's step"""
        self._note("red", *self._close(13))
        P, = self.powers()
        self._note("sum", *self.sums)
        self._note("P", P)
        if self._tick():
            self._point(k, P, self._centre, self._symbol)

    def status(self):
        """kq_psk_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, shreg=self.shreg, over=self.over, events=self.nevents,
                    dropped=self.dropped, reserved=0, sig=self.sig, qre=self.qre, qim=self.qim, ee=self.Ee, el=self.El,
                    pe=self.Pe, pc=self.Pc, rot_r=self.R[0], rot_i=self.R[1], cr=self.c[0], ci=self.c[1], pr=self.p[0], pi=self.p[1],
                    sum_i=self.sums[0], sum_q=self.sums[1], acc_i=self.acc[0], acc_q=self.acc[1])
