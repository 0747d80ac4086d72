"""The front half that the models of the frame-grid decoders share (cw_model, rtty_model, psk_model, ale_model, dsc_model),
the model side of ka9q_sdr_amd/csrc/kq_tonecorr.hpp: the quantiser of fsk_model, tone_model's cosine table, NT correlators
whose phases are functions of the sample index alone, the open frame's sums in int64 (exact: they stay below 2^42), the
shift that reduces a completed frame's sums, the window W frames long over the reduced sums, the early / centre / late
clock (tc::clock_adjust), the levels and the gate of a bit of dsc_model, navtex_model and same_model (tc::bit_levels), and
the arena's saturating counts.  Everything behind the quantiser is Python ints.

What a model still writes: its tracker (`_frame`, and the centre and late points where it has a clock), `status()`, STATUS and
Event."""
import collections
import math

import numpy as np

import fsk_model as fm
import tone_model as tm

TABLE = tm.TABLE
cos_table = tm.cos_table
M32 = 0xFFFFFFFF


def inc(f, Fs):
    """inc = rint(f 2^32 / Fs) in double, f a float32"""
    return int(np.rint(float(np.float32(f)) * 4294967296.0 / float(Fs)))


def period(Fs, B, baud):
    """tb = rint(256 Fs / (B baud)) in double, baud a float32: the bit or symbol in 1/256 frame"""
    return int(np.rint(256.0 * float(Fs) / (float(B) * float(np.float32(baud)))))


def window(tb):
    """W = (tb + 128) >> 8 frames"""
    return (tb + 128) >> 8


def pairs(v):
    """[[I, Q] of tone 0, [I, Q] of tone 1, ...] of a flat list"""
    return [list(v[c:c + 2]) for c in range(0, len(v), 2)]


def noise_sigma(amp, db, Fs, baud):
    """white noise that leaves a tone of amplitude amp at Eb/N0 (Es/N0) of `db`: sigma^2 = (amp^2 / 2) / 10^(dB / 10)
    Fs / (2 baud)"""
    return math.sqrt(amp * amp / 2.0 / 10.0 ** (db / 10.0) * float(Fs) / (2.0 * float(baud)))


class GridModel:
    """one slot's front half.  incs: a phase increment per tone; acc, sums: I, Q of tone 0, I, Q of tone 1, ...; tb: the
    period in 1/256 frame, or None where the decoder slides no window (cw_model); start: the sample at which the slot was
    set (x = 0 before it).  `widest` records every intermediate by kind, so that a test can hold each inside the bound
    the header states."""

    def __init__(self, samprate, block_len, incs, table, tb, input_scale, max_events, start, widest=()):
        self.Fs, self.B = float(samprate), int(block_len)
        self.scale, self.max_events = input_scale, max_events
        self.C = cos_table() if table is None else np.asarray(table, np.int16)
        self.incs = tuple(int(v) for v in incs)
        self.n = int(start)
        self.acc = [0] * (2 * len(self.incs))                       # the open frame
        self.frames = self.nevents = self.dropped = 0
        self.events = []
        self.widest = dict.fromkeys(("acc", "red", "sum") + tuple(widest), 0)
        if tb is not None:
            self.tb = int(tb)
            self.W = window(self.tb)
            self.q = self.tb >> 2
            self.hist = collections.deque([(0,) * len(self.acc)] * self.W, self.W)   # the last W frames' reduced sums
            self.sums = [0] * len(self.acc)
            self.ph = self.t = self.Ee = self.El = self.Pe = 0      # the clock, where the decoder has one

    def feed(self, x, s16=False):
        q = fm.quantise(x, self.scale, s16)
        if not len(q):
            return self
        B, n0 = self.B, self.n
        n = np.arange(n0, n0 + len(q), dtype=np.uint64)
        Ct = self.C.astype(np.int64)
        cuts = np.concatenate([[0], np.arange(B - n0 % B, len(q), B)]).astype(np.int64)     # where the chunk's frames begin
        ends = np.concatenate([cuts[1:], [len(q)]]).tolist()
        part = []
        for v in self.incs:
            j = (((n * np.uint64(v)) & np.uint64(M32)) >> np.uint64(22)).astype(np.int64)   # mod 2^64 keeps mod 2^32
            part.append(np.add.reduceat(q * Ct[j], cuts).tolist())                          # exact: int64
            part.append(np.add.reduceat(q * Ct[(j - 256) & (TABLE - 1)], cuts).tolist())
        for i, e in enumerate(ends):
            for c in range(len(part)):
                self.acc[c] += part[c][i]
            self.n = n0 + e
            if self.n % B == 0:
                self._frame(self.n // B - 1)
        return self

    def _note(self, kind, *values):
        self.widest[kind] = max(self.widest[kind], *(abs(v) for v in values))

    def _close(self, shift):
        """the open frame completes: its sums reduced by `shift` enter the window; returns them"""
        red = tuple(v >> shift for v in self.acc)
        self._note("acc", *self.acc)
        self.acc = [0] * len(self.acc)
        old = self.hist[0]
        self.hist.append(red)
        self.sums = [s + a - o for s, a, o in zip(self.sums, red, old)]
        self.frames = min(self.frames + 1, M32)
        return red

    def powers(self):
        """I^2 + Q^2 of the window's sums, per tone"""
        return [self.sums[c] ** 2 + self.sums[c + 1] ** 2 for c in range(0, len(self.sums), 2)]

    def _tick(self):
        """a frame passes: True at a point of the clock"""
        self.t -= 256
        return self.t < 128

    def _point(self, k, P, centre, late):
        """a point of the clock at frame k, P the power it tracks: the early point keeps P, the centre is the decoder's
        centre(P), and at the late one its late(k, P) reads the symbol"""
        if self.ph == 2:
            self.ph = 0
            late(k, P)
            return
        if self.ph == 0:
            self.Pe = P
        else:
            centre(P)
        self.t += self.q
        self.ph += 1

    def _timing(self, Pl):
        """the late point's timing update: early against late, a step of tb / 32 where they differ by more than an eighth;
        returns (adj, the larger of the two)"""
        tb = self.tb
        self.Ee += (self.Pe - self.Ee) >> 3
        self.El += (Pl - self.El) >> 3
        m = max(self.Ee, self.El)
        adj = 0
        if self.Ee > self.El and self.Ee - self.El > (m >> 3):
            adj = -(tb >> 5)
        elif self.El > self.Ee and self.El - self.Ee > (m >> 3):
            adj = tb >> 5
        self.t += tb - 2 * self.q + adj
        return adj, m

    def _levels(self, Pl, nudge=True):
        """steps 1 and 2 of a bit of the two-tone decoders with a bit clock, at its late point (tc::bit_levels): the timing, the
        centre level Ec and the push of tb / 32 where the clock stands half a bit out (no slope there; nudge=False leaves it
        out), the levels sig and nse of the centre's hi and lo, and the gate over the model's warm, min_p and snr, which its
        gate=False leaves open; returns whether it is open"""
        adj, m = self._timing(Pl)
        self.Ec += (self.hi - self.Ec) >> 3
        if nudge and adj == 0 and self.Ec + (m >> 3) < min(self.Ee, self.El):
            self.t += self.tb >> 5
        self.sig += (self.hi - self.sig) >> 4
        self.nse += (self.lo - self.nse) >> 4
        is_open = self.frames >= self.warm and self.sig >= self.min_p and 16 * self.sig >= self.snr * self.nse
        return is_open or not self.gate

    def _file(self, event):
        self.nevents = min(self.nevents + 1, M32)
        if len(self.events) >= self.max_events:
            self.dropped = min(self.dropped + 1, M32)
        else:
            self.events.append(event)

    def clear_events(self):
        self.events = []
