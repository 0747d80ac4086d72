"""The ACARS decoder of include/ka9q_hip.h (kq_acars_*) restated in numpy and Python ints, for the tests: kq_fsk_*'s
quantiser, kq_cw_*'s cosine table, the mixer whose phase is a function of the sample index alone, the matched filter at
every sample, the correlation against the 40 preamble bits with its threshold and its local maximum, and the walk of
an open block's bits: decision, rotation, early / late timing, characters, parity, CRC and the close.  The sums are int64
(the header's bounds keep them inside), the walk is Python ints; there is no float after the quantiser.  The geometry
becomes integers before any sample is seen, by the header's formulas in double.  The model carries its own parity and
CRC.  Every intermediate's widest value is kept in `widest`, by kind."""
import collections

import numpy as np

TABLE = 1024
BAUD = 2400.0
SHIFT = 30
PRE = (0x2b, 0x2a, 0x16, 0x16, 0x01)
ETX, ETB = 0x03, 0x17
GOOD, BY_ETB, OVERRUN = 1, 2, 4
STATUS = ("syncs", "blocks_good", "blocks_bad", "overruns", "dropped", "discarded", "in_block", "k", "nbits", "cur", "length",
          "parity_errors", "crc", "ending", "cnt", "reserved", "t", "search_from", "acc", "sync_sample", "sync_c2", "sync_e", "rr",
          "ri")
Record = collections.namedtuple("Record", "data length flags parity_errors sync_sample end_sample sync_c2 sync_e r2")


def cos_table():
    """C[j] = rint(32767 cos(2 pi j / 1024)) in double: kq_cw_*'s table"""
    return np.rint(32767.0 * np.cos(2.0 * np.pi * np.arange(TABLE) / TABLE)).astype(np.int16)


def quantise(x, scale, s16=False):
    """q: float32 multiply, round to nearest even, clamp; NaN reads as 0.  s16: int16 words taken as they are"""
    if s16:
        return np.maximum(np.asarray(x).astype(np.int64), -32767)
    v = np.rint(np.asarray(x, np.float32) * np.float32(scale))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, -32767, 32767).astype(np.int64)


def odd(c):
    """bit 7 makes the parity odd"""
    c &= 0x7f
    return c | (0x80 if bin(c).count("1") % 2 == 0 else 0)


def crc16(data):
    r = 0
    for b in bytes(data):
        for i in range(8):
            r = (r >> 1) ^ (0x8408 if (r ^ (b >> i)) & 1 else 0)
    return r


def pattern():
    """d_k = +-1 of the 40 preamble bits, parity bits included, least significant bit first"""
    return [2 * ((odd(c) >> i) & 1) - 1 for c in PRE for i in range(8)]


class Geom:
    """the integers a sample rate makes"""

    def __init__(self, Fs):
        Fs = float(Fs)
        self.Fs = Fs
        self.inc = int(np.rint(1800.0 * 4294967296.0 / Fs))
        self.FL = int(np.rint(2.0 * Fs / BAUD))
        self.hq = np.rint(32767.0 * np.cos(np.pi * (np.arange(self.FL) - (self.FL - 1) / 2.0) / self.FL)).astype(np.int64)
        self.w = int(np.ceil(Fs / BAUD))
        self.e = max(1, int(np.rint(Fs / 9600.0)))
        self.tb = int(np.rint(256.0 * Fs / BAUD))
        self.off = [int(np.rint((k - 39) * Fs / BAUD)) for k in range(40)]
        self.H39 = -self.off[0]
        self.HA = self.H39 + 2 * self.w          # values of a in front of a call's first sample
        self.H = self.HA + self.FL - 1           # values of q carried


def turn(ar, ai, m):
    """(ar + j ai) (-j)^m"""
    m &= 3
    return ((ar, ai), (ai, -ar), (-ar, -ai), (-ai, ar))[m]


class AcarsModel:
    """one slot.  table, taps: the bank's own (kq_cw_get_table's values, kq_acars_get_taps), or None for the model's;
    start: the sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, input_scale=32767.0, sync_num=1, sync_den=2, max_parity_errors=3, max_block_bytes=256,
                 max_blocks=16, table=None, taps=None, start=0):
        self.g = g = Geom(samprate)
        self.scale = input_scale
        self.num, self.den, self.mpe, self.mbb, self.max_blocks = sync_num, sync_den, max_parity_errors, max_block_bytes, max_blocks
        self.C = (cos_table() if table is None else np.asarray(table, np.int16)).astype(np.int64)
        self.hq = g.hq if taps is None else np.asarray(taps, np.int64)
        assert len(self.hq) == g.FL
        self.d = pattern()
        self.n = int(start)
        self.q = np.zeros(g.H, np.int64)
        self.syncs = self.blocks_good = self.blocks_bad = self.overruns = self.dropped = self.discarded = 0
        self.in_block = self.k = self.nbits = self.cur = self.length = self.parity_errors = self.crc = self.ending = self.cnt = 0
        self.t = self.search_from = self.acc = self.sync_sample = self.sync_c2 = self.sync_e = self.rr = self.ri = 0
        self.open = bytearray()
        self.blocks = []
        self.nfiled = 0              # in the arena since the last clear
        self.best = (0, 1)           # the largest sync metric seen, as (|c|^2, 40 e)
        self.bits = []
        self.widest = dict(z=0, v=0, a=0, c=0, c2=0, e=0, lhs=0, rhs=0, dot=0, acc=0, R=0, r2=0)

    def _wide(self, kind, v):
        if v > self.widest[kind]:
            self.widest[kind] = int(v)

    def clear_blocks(self):
        self.nfiled = 0
        self.blocks = []

    def status(self):
        s = {k: int(getattr(self, k, 0)) for k in STATUS}
        return s

    # ---- the parallel half: a, c, |c|^2, e and the sync flags of a call --------------------------------------------------
    def _front(self, q):
        """q: the carried H values and the call's.  Returns a (from n0 - HA), c, c2, e (from n0 - 2 w)"""
        g = self.g
        first = self.n - g.H                                   # the index of q[0]
        n = (np.arange(first, first + len(q), dtype=np.int64)).astype(np.uint64)
        j = (((n * np.uint64(g.inc)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
        zr, zi = q * self.C[j], -q * self.C[(j - 256) & (TABLE - 1)]
        m = len(q) - (g.FL - 1)
        vr, vi = np.zeros(m, np.int64), np.zeros(m, np.int64)
        for i in range(g.FL):                                  # v[n] = sum hq[i] z[n - i]
            lo = g.FL - 1 - i
            vr += self.hq[i] * zr[lo:lo + m]
            vi += self.hq[i] * zi[lo:lo + m]
        ar, ai = vr >> SHIFT, vi >> SHIFT
        if len(q):
            self._wide("z", max(np.abs(zr).max(), np.abs(zi).max()))
            self._wide("v", max(np.abs(vr).max(), np.abs(vi).max()))
            self._wide("a", max(np.abs(ar).max(), np.abs(ai).max()))
        mc = m - g.H39                                         # c from n0 - 2 w
        cr, ci, e = np.zeros(mc, np.int64), np.zeros(mc, np.int64), np.zeros(mc, np.int64)
        for k in range(40):
            lo = g.H39 + g.off[k]
            xr, xi = turn(ar[lo:lo + mc], ai[lo:lo + mc], k)
            cr += self.d[k] * xr
            ci += self.d[k] * xi
            e += ar[lo:lo + mc] ** 2 + ai[lo:lo + mc] ** 2
        c2 = cr * cr + ci * ci
        if mc > 0:
            self._wide("c", max(np.abs(cr).max(), np.abs(ci).max()))
            self._wide("c2", c2.max())
            self._wide("e", e.max())
        return ar, ai, cr, ci, c2, e

    def feed(self, x, s16=False):
        g = self.g
        new = quantise(x, self.scale, s16)
        q = np.concatenate([self.q, new])
        n0, n1 = self.n, self.n + len(new)
        ar, ai, cr, ci, c2, e = self._front(q)
        abase, cbase = n0 - g.HA, n0 - 2 * g.w                  # the index of a[0] and of c[0]
        # flags for p in [n0 - w, n1 - w)
        lo, m = g.w, len(new)
        lhs, rhs = c2[lo:lo + m] * self.den, e[lo:lo + m] * (40 * self.num)
        if m:
            self._wide("lhs", lhs.max())
            self._wide("rhs", rhs.max())
            ok = e[lo:lo + m] > 0
            if ok.any():
                i = int(np.argmax(np.where(ok, c2[lo:lo + m] / np.maximum(e[lo:lo + m], 1), 0.0)))
                if int(c2[lo + i]) * self.best[1] > self.best[0] * 40 * int(e[lo + i]):
                    self.best = (int(c2[lo + i]), 40 * int(e[lo + i]))
        cand = np.nonzero((lhs >= rhs) & (c2[lo:lo + m] > 0))[0]
        flags = []
        for i in cand:
            v = c2[lo + i]
            if (c2[lo + i - g.w:lo + i] < v).all() and (c2[lo + i + 1:lo + i + g.w + 1] <= v).all():
                flags.append(n0 - g.w + int(i))
        # the walk over p in [n0 - w, n1 - w)
        limit = n1 - g.w
        fi = 0
        while True:
            if self.in_block:
                nb = (self.t + g.tb + 128) >> 8
                if nb >= limit:
                    break
                self._bit(nb, ar, ai, abase)
            else:
                while fi < len(flags) and flags[fi] < self.search_from:
                    fi += 1
                if fi == len(flags):
                    break
                p = flags[fi]
                fi += 1
                self.syncs += 1
                self.in_block = 1
                self.rr, self.ri = int(cr[p - cbase]) >> 5, int(ci[p - cbase]) >> 5
                self.t, self.k = p << 8, 39
                self.sync_sample, self.sync_c2, self.sync_e = p, int(c2[p - cbase]), int(e[p - cbase])
                self.nbits = self.cur = self.length = self.parity_errors = self.crc = self.ending = self.cnt = self.acc = 0
                self.open = bytearray()
        self.q = q[len(q) - g.H:]
        self.n = n1

    # ---- the serial half ------------------------------------------------------------------------------------------------
    def _bit(self, n, ar, ai, abase):
        g = self.g
        self.t += g.tb
        self.k = (self.k + 1) & 0xFFFFFFFF
        ur, ui = turn(int(ar[n - abase]), int(ai[n - abase]), self.k)
        dot = ur * self.rr + ui * self.ri
        bit = 1 if dot >= 0 else 0
        er, ei = turn(int(ar[n - g.e - abase]), int(ai[n - g.e - abase]), self.k)
        lr, li = turn(int(ar[n + g.e - abase]), int(ai[n + g.e - abase]), self.k)
        de, dl = abs(er * self.rr + ei * self.ri), abs(lr * self.rr + li * self.ri)
        self._wide("dot", max(abs(dot), de, dl))
        self.acc += de - dl
        self._wide("acc", abs(self.acc))
        s = 1 if bit else -1
        self.rr += (s * ur - self.rr) >> 4
        self.ri += (s * ui - self.ri) >> 4
        self._wide("R", max(abs(self.rr), abs(self.ri)))
        self.cnt += 1
        if self.cnt == 8:
            r2 = self.rr * self.rr + self.ri * self.ri
            self._wide("r2", r2)
            if 4 * self.acc > r2:
                self.t -= g.tb >> 5
            elif 4 * self.acc < -r2:
                self.t += g.tb >> 5
            self.acc = self.cnt = 0
        self.bits.append(bit)
        # the frame
        self.cur |= bit << self.nbits
        self.crc = (self.crc >> 1) ^ (0x8408 if (self.crc ^ bit) & 1 else 0)
        self.nbits += 1
        if self.nbits < 8:
            return
        byte, self.cur, self.nbits = self.cur, 0, 0
        self.open.append(byte)
        self.length += 1
        if self.ending:                                        # bytes of the check left, + 4 behind an ETB
            self.ending -= 1
            if (self.ending & 3) == 0:
                self._close(n, (GOOD if self.crc == 0 else 0) | (BY_ETB if self.ending & 4 else 0))
                self.ending = 0
            return
        if bin(byte).count("1") % 2 == 0:
            self.parity_errors += 1
        if (byte & 0x7f) in (ETX, ETB) and self.length <= self.mbb - 2:
            self.ending = 6 if (byte & 0x7f) == ETB else 2
        elif self.length >= self.mbb - 2:
            self._close(n, OVERRUN)

    def _close(self, n, flags):
        if flags & GOOD:
            self.blocks_good += 1
        elif flags & OVERRUN:
            self.overruns += 1
        else:
            self.blocks_bad += 1
        if flags & GOOD or self.parity_errors <= self.mpe:
            if self.nfiled < self.max_blocks:
                r2 = self.rr * self.rr + self.ri * self.ri
                self.blocks.append(Record(bytes(self.open), self.length, flags, self.parity_errors, self.sync_sample, n,
                                          self.sync_c2, self.sync_e, r2))
                self.nfiled += 1
            else:
                self.dropped += 1
        else:
            self.discarded += 1
        self.in_block = 0
        self.search_from = n + 1


def noise_sigma(amp, ebn0_db, Fs):
    """sigma of white noise per sample for an Eb/N0: sigma^2 = (amp^2 / 2 / 2400) / 10^(dB / 10) Fs / 2"""
    return float(np.sqrt((amp * amp / 2.0 / BAUD) / 10.0 ** (ebn0_db / 10.0) * Fs / 2.0))
