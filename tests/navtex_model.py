"""The NAVTEX decoder of include/ka9q_hip.h (kq_navtex_*) restated in numpy and Python ints, for the tests, from the
header's text: grid_model's front half and clock (kq_dsc_*'s: the quantiser, the cosine table, two correlators whose phases
are functions of the sample index alone, the window one bit long, the early / centre / late clock with its push from half
a bit out, the levels and the gate), then the 128-bit register, the attempt on the phasing signals and on running traffic,
on the register and on its complement, and in sync a character at every RX place resolved from its DX and its RX copy.
Everything from the shifts on is Python ints: there is no float after the quantiser."""
import collections

import fsk_model as fm            # (the tests reach the quantiser through the model: fm.quantise)
import grid_model as gm

TABLE = gm.TABLE
M128 = (1 << 128) - 1
M64 = (1 << 64) - 1
ALPHA, BETA, REP, NONE = 0x78, 0x66, 0x33, 0x7F
UNRESOLVED, FROM_RX, DIFFER, INVERTED = 1, 2, 4, 8
Event = collections.namedtuple("Event", "code flags dx rx end_sample sig nse")
STATUS = ("frames", "ph", "t", "bit", "nbits", "synced", "bitpos", "kind", "inverted", "run", "events", "dropped", "syncs",
          "tsyncs", "losses", "idles", "sig", "nse", "ee", "el", "ec", "pe", "hi", "lo", "r_hi", "r_lo", "sum", "acc")

cos_table, navtex_inc, bit_length, window = gm.cos_table, gm.inc, gm.period, gm.window


def is_char(w):
    return bin(w).count("1") == 4


def phasing(x, acq):
    """the header's step 4, the phasing signals on x: 1 the latest place is RX, 0 it is DX, -1 no sync"""
    c = [x >> (7 * i) & 127 for i in range(4)]
    as_rx = sum(c[i] == (ALPHA, REP)[i & 1] for i in range(4))
    as_dx = sum(c[i] == (REP, ALPHA)[i & 1] for i in range(4))
    return 1 if as_rx >= acq else 0 if as_dx >= acq else -1


def traffic(x, pairs):
    """the header's step 4, running traffic on x"""
    seen = set()
    for j in range(pairs):
        rx, dx = x >> (14 * j) & 127, x >> (14 * j + 35) & 127
        if rx != dx or not is_char(rx) or rx in (ALPHA, BETA, REP):
            return False
        seen.add(rx)
    return len(seen) >= 2


class NavtexModel(gm.GridModel):
    """one slot.  table, incs, tb: the bank's own (kq_navtex_get_table, kq_navtex_get_slot), or None for the model's; start:
    the sample at which the slot was set (x = 0 before it).  gate=False leaves the gate open (the model only: for the
    false-alarm tests)"""

    def __init__(self, samprate, block_len, mark=1785.0, space=1615.0, baud=100.0, warm=64, snr=64, min_p=1 << 16, acq=4, pairs=4,
                 lose=16, input_scale=32767.0, max_events=512, table=None, incs=None, tb=None, start=0, gate=True):
        incs = (navtex_inc(mark, samprate), navtex_inc(space, samprate)) if incs is None else incs   # mark, then space
        super().__init__(samprate, block_len, incs, table, bit_length(samprate, block_len, baud) if tb is None else tb, input_scale,
                         max_events, start, widest=("P",))
        self.warm, self.snr, self.min_p = int(warm), int(snr), int(min_p)
        self.acq, self.pairs, self.lose, self.gate = int(acq), int(pairs), int(lose), gate
        self.bit = self.nbits = self.synced = self.bitpos = self.kind = self.inverted = self.run = 0
        self.Ec = self.sig = self.nse = self.hi = self.lo = self.r = 0
        self.syncs = self.tsyncs = self.losses = self.idles = 0
        self.bits = []               # of every bit: (bit, open)

    def _centre(self, best):
        Pm, Ps = self.powers()
        self.bit, self.hi, self.lo = int(Pm >= Ps), best, min(Pm, Ps)

    def _bit(self, k, Pl):
        """the header's steps 1 to 5 at a late point, frame k"""
        is_open = self._levels(Pl)  # 1 timing, 2 levels and gate
        self.bits.append((self.bit, is_open))
        # 3 register
        self.r = (self.r << 1 | self.bit) & M128
        self.nbits = (self.nbits + 1) & 0xFFFFFFFF
        # 4 sync
        if not self.synced:
            if not is_open:
                return
            for inv, x in ((0, self.r), (1, self.r ^ M128)):
                kind, by_traffic = phasing(x, self.acq), False
                if kind < 0 and traffic(x, self.pairs):
                    kind, by_traffic = 1, True
                if kind >= 0:
                    break
            else:
                return
            self.synced, self.bitpos, self.kind, self.inverted, self.run = 1, 0, kind, inv, 0
            if by_traffic:
                self.tsyncs = min(self.tsyncs + 1, 0xFFFFFFFF)
            else:
                self.syncs = min(self.syncs + 1, 0xFFFFFFFF)
            return
        # 5 characters
        self.bitpos += 1
        if self.bitpos < 7:
            return
        self.bitpos = 0
        self.kind ^= 1
        if not self.kind:
            return
        x = self.r ^ M128 if self.inverted else self.r
        dx, rx = x >> 35 & 127, x & 127
        if (dx == REP and rx == ALPHA) or (is_char(dx) and is_char(rx) and dx == rx):
            self.run = 0
        else:
            self.run += 1
        if dx == REP or rx == ALPHA:
            self.idles = min(self.idles + 1, 0xFFFFFFFF)
        else:
            if is_char(dx):
                code, flags = dx, DIFFER if is_char(rx) and rx != dx else 0
            elif is_char(rx):
                code, flags = rx, FROM_RX
            else:
                code, flags = NONE, UNRESOLVED
            self._file(Event(code, flags | (INVERTED if self.inverted else 0), dx, rx, (k + 1) * self.B, self.sig, self.nse))
        if self.run >= self.lose:
            self.synced = 0
            self.losses = min(self.losses + 1, 0xFFFFFFFF)

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
        """kq_navtex_status: everything carried but the past frames"""
        return dict(frames=self.frames, ph=self.ph, t=self.t, bit=self.bit, nbits=self.nbits, synced=self.synced,
                    bitpos=self.bitpos, kind=self.kind, inverted=self.inverted, run=self.run, events=self.nevents,
                    dropped=self.dropped, syncs=self.syncs, tsyncs=self.tsyncs, losses=self.losses, idles=self.idles,
                    sig=self.sig, nse=self.nse, ee=self.Ee, el=self.El, ec=self.Ec, pe=self.Pe, hi=self.hi, lo=self.lo,
                    r_hi=self.r >> 64, r_lo=self.r & M64, sum=gm.pairs(self.sums), acc=gm.pairs(self.acc))


def noise_sigma(amp, esn0_db, Fs, baud=100.0):
    return gm.noise_sigma(amp, esn0_db, Fs, baud)
