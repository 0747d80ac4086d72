"""The RTTY decoder of include/ka9q_hip.h (kq_rtty_*) restated in numpy and Python ints, for the tests: the quantiser of
fsk_model, tone_model's cosine table, two correlators whose phases are functions of the sample index alone, a sliding
window one bit long over the frames' reduced sums, and the start-stop framer, a step per completed frame.  The frame sums
are taken in int64 (they stay below 2^38) and everything from the shifts on in Python ints: there is no float after the
quantiser.  The bit length becomes an integer (tb) before any sample is seen, by the header's formula in double.  Every
intermediate is recorded in `widest`, by kind, so that a test can hold each inside the bound the header states."""
import collections

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
WAIT, IDLE, CHAR = 0, 1, 2
Event = collections.namedtuple("Event", "code flags start_sample sig nse")
STATUS = ("frames", "state", "bit", "code", "t", "events", "dropped", "ferr", "false_starts", "reserved", "sig", "nse", "start",
          "sum_im", "sum_qm", "sum_is", "sum_qs", "acc_im", "acc_qm", "acc_is", "acc_qs")

cos_table, rtty_inc, bit_length, window, noise_sigma = gm.cos_table, gm.inc, gm.period, gm.window, gm.noise_sigma


class RttyModel(gm.GridModel):
    """one slot.  table, incs, tb: the bank's own (kq_rtty_get_table, kq_rtty_get_slot), or None for the model's; start:
    the sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, mark=2125.0, space=2295.0, baud=45.45, nbits=5, warm=64, snr=96, min_p=1 << 16,
                 input_scale=32767.0, max_events=256, table=None, incs=None, tb=None, start=0):
        incs = (rtty_inc(mark, samprate), rtty_inc(space, samprate)) if incs is None else incs   # mark, then space
        super().__init__(samprate, block_len, incs, table, bit_length(samprate, block_len, baud) if tb is None else tb, input_scale,
                         max_events, start, widest=("P", "lvl", "prod"))
        self.nbits, self.warm, self.snr, self.min_p = int(nbits), int(warm), int(snr), int(min_p)
        self.sig = self.nse = 0
        self.state, self.bit, self.code, self.t, self.start = WAIT, 0, 0, 0, 0
        self.ferr = self.false_starts = 0
        self.levels = []             # of every completed frame

    def _frame(self, k):
        """the header's steps 1 to 4 on frame k, behind the window"""
        self._note("red", *self._close(12))
        Pm, Ps = self.powers()
        self._note("sum", *self.sums)
        self._note("P", Pm, Ps)
        # 1 count (the window's) and level
        hi, lo, lev = max(Pm, Ps), min(Pm, Ps), int(Pm >= Ps)
        self.levels.append(lev)
        # 2 levels
        samp = self.state == CHAR and self.t - 256 < 128
        if self.state != CHAR or samp:
            sh = 4 if samp else 6
            self.sig += (hi - self.sig) >> sh
            self.nse += (lo - self.nse) >> sh
            self._note("lvl", self.sig, self.nse)
        # 3 validity
        self._note("prod", 16 * self.sig, self.nse * self.snr)
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
                self._file(Event(self.code, 0, self.start * self.B, self.sig, self.nse))
                self.state = IDLE
            else:
                self._file(Event(self.code, 1, self.start * self.B, self.sig, self.nse))
                self.ferr = min(self.ferr + 1, 0xFFFFFFFF)
                self.state = WAIT

    def status(self):
        """kq_rtty_status: every counter, the framer and level state, the window sums and the open frame's sums"""
        return dict(frames=self.frames, state=self.state, bit=self.bit, code=self.code, t=self.t, events=self.nevents,
                    dropped=self.dropped, ferr=self.ferr, false_starts=self.false_starts, reserved=0, sig=self.sig,
                    nse=self.nse, start=self.start, sum_im=self.sums[0], sum_qm=self.sums[1], sum_is=self.sums[2],
                    sum_qs=self.sums[3], acc_im=self.acc[0], acc_qm=self.acc[1], acc_is=self.acc[2], acc_qs=self.acc[3])
