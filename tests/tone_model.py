"""The tone signalling decoder of include/ka9q_hip.h (kq_tone_*) restated in numpy and Python ints, for the tests: the
quantiser of fsk_model, the cosine table, correlators whose phase is a function of the sample index alone, the decision per
block and the runs.  The block sums are taken in int64 (they stay below 2^43) and everything from the shifts on in Python
ints, with every intermediate of the decision recorded in `widest`, so that a test can see none of them leave 64 bits."""
import collections

import numpy as np

import fsk_model as fm
from ka9q_sdr_amd import selcall as sc

TABLE = 1024
Event = collections.namedtuple("Event", "symbol blocks start_sample peak")
STATUS = ("blocks", "valid_blocks", "events", "dropped", "cur", "run", "energy")


def cos_table():
    """C[j] = rint(32767 cos(2 pi j / 1024)) in double"""
    return np.rint(32767.0 * np.cos(2.0 * np.pi * np.arange(TABLE) / TABLE)).astype(np.int16)


def tone_incs(freqs, Fs):
    """inc_t = rint(f_t 2^32 / Fs) in double, f_t a float32"""
    return np.rint(np.asarray(freqs, np.float32).astype(np.float64) * 4294967296.0 / float(Fs)).astype(np.uint32)


def block_sums(q, n0, incs, C):
    """I_t, Q_t, E of the samples q at n0, n0 + 1, ...: Python ints"""
    q = np.asarray(q, np.int64)
    n = np.arange(n0, n0 + len(q), dtype=np.uint64)
    ph = (n[:, None] * np.asarray(incs, np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)     # wraps mod 2^64: mod 2^32 is kept
    j = (ph >> np.uint64(22)).astype(np.int64)
    Ct = np.asarray(C, np.int64)
    I = (q[:, None] * Ct[j]).sum(0)
    Q = (q[:, None] * Ct[(j - 256) & (TABLE - 1)]).sum(0)
    return [int(v) for v in I], [int(v) for v in Q], int((q * q).sum())


def powers(I, Q):
    """P_t = (I_t >> 15)^2 + (Q_t >> 15)^2 (Python's >> on ints is the arithmetic shift)"""
    return [(i >> 15) ** 2 + (q >> 15) ** 2 for i, q in zip(I, Q)]


def decide(P, E, B, groups, min_ms, frac, ratio, twist, widest=None):
    """the symbol of a completed block, or -1; `widest`: a list that takes every intermediate"""
    seen = widest if widest is not None else []
    R = E * B
    floor = (R >> 8) * frac
    seen += [R, floor, min_ms * B]
    ok = E >= min_ms * B
    lo, sym, best = 0, 0, []
    for g, cnt in enumerate(c for c in groups if c):
        grp = P[lo:lo + cnt]
        pb = max(grp)
        i = grp.index(pb)                                   # the lowest index that attains it
        p2 = max(grp[:i] + grp[i + 1:], default=0)
        seen += [pb, (p2 >> 4) * ratio]
        ok = ok and pb >= floor and pb >= (p2 >> 4) * ratio
        sym |= i << (8 * g)
        best.append(pb)
        lo += cnt
    if len(best) == 2:
        seen.append((min(best) >> 4) * twist)
        ok = ok and max(best) <= (min(best) >> 4) * twist
    return sym if ok else -1


class ToneModel:
    """one slot.  table, incs: the bank's own (kq_tone_get_table, kq_tone_get_incs), or None for the model's; start: the
    sample at which the slot was set (x = 0 before it)"""

    def __init__(self, samprate, block_len, freqs, groups, min_ms=16, frac=None, ratio=64, twist=160, min_blocks=2,
                 input_scale=32767.0, max_events=64, table=None, incs=None, start=0):
        self.Fs, self.B = float(samprate), int(block_len)
        self.groups = tuple(groups)
        self.T = len(freqs)
        assert sum(self.groups) == self.T
        self.min_ms, self.ratio, self.twist, self.min_blocks = min_ms, ratio, twist, min_blocks
        self.frac = (16 if len([g for g in self.groups if g]) == 2 else 64) if frac is None else frac
        self.scale, self.max_events = input_scale, max_events
        self.C = cos_table() if table is None else np.asarray(table, np.int16)
        self.incs = tone_incs(freqs, samprate) if incs is None else np.asarray(incs, np.uint32)
        self.n = int(start)
        self.I, self.Q, self.E = [0] * self.T, [0] * self.T, 0
        self.cur, self.run, self.start, self.peak = -1, 0, 0, 0
        self.blocks = self.valid = self.nevents = self.dropped = 0
        self.last_P, self.last_E = [0] * self.T, 0
        self.events = []
        self.symbols = []            # of every completed block
        self.widest = []

    def _block(self, k):
        P, E = powers(self.I, self.Q), self.E
        s = decide(P, E, self.B, self.groups, self.min_ms, self.frac, self.ratio, self.twist, self.widest)
        self.widest += [abs(v) for v in self.I + self.Q] + P
        self.symbols.append(s)
        self.blocks += 1
        self.valid += s >= 0
        self.last_P, self.last_E = P, E
        self.I, self.Q, self.E = [0] * self.T, [0] * self.T, 0
        if s == self.cur:
            self.run = min(self.run + 1, 0xFFFFFFFF)
            self.peak = max(self.peak, E)
            return
        if self.cur >= 0 and self.run >= self.min_blocks:
            self.nevents += 1
            if len(self.events) >= self.max_events:
                self.dropped += 1
            else:
                self.events.append(Event(self.cur, self.run, self.start * self.B, self.peak))
        self.cur, self.run, self.start, self.peak = s, 1, k, E

    def feed(self, x, s16=False):
        q = fm.quantise(x, self.scale, s16)
        at = 0
        while at < len(q):
            k = self.n // self.B
            m = min(len(q) - at, (k + 1) * self.B - self.n)
            I, Q, E = block_sums(q[at:at + m], self.n, self.incs, self.C)
            self.I = [a + b for a, b in zip(self.I, I)]
            self.Q = [a + b for a, b in zip(self.Q, Q)]
            self.E += E
            self.n += m
            at += m
            if self.n == (k + 1) * self.B:
                self._block(k)
        return self

    def status(self):
        return dict(blocks=self.blocks, valid_blocks=self.valid, events=self.nevents, dropped=self.dropped, cur=self.cur,
                    run=self.run, energy=self.last_E)

    def powers(self):
        """the powers plane's row: P_t of the last completed block, then its E"""
        return self.last_P + [self.last_E]

    def clear_events(self):
        self.events = []


def dtmf_train(Fs, B, seed, twist_db):
    """test traffic: 16 random keys, 50 ms on and 50 ms off, from a random offset within a block behind one block of
    silence; each key's tones off by up to +-1.5 %; white noise 20 dB below the low tone.  (keys, lead in seconds, audio)"""
    rng = np.random.default_rng(seed)
    keys = "".join(rng.choice(list(sc.DTMF.keys), 16))
    lead = (B + int(rng.integers(0, B))) / Fs
    x = sc.dtmf_encode(keys, Fs, 0.050, 0.050, twist_db, lead=lead, ferr=rng.uniform(-0.015, 0.015, 16), noise_db=20.0,
                       seed=seed)
    return keys, lead, x


def zvei_train(Fs, B, seed, plan=sc.ZVEI1):
    """five random digits (every fourth train with a repeated one) as one call, noise 12 dB down: (digits, lead, audio)"""
    rng = np.random.default_rng(seed)
    digits = "".join(rng.choice(list("0123456789"), 5))
    if seed % 4 == 0:
        digits = digits[:2] + digits[1] + digits[3:]
    lead = (B + int(rng.integers(0, B))) / Fs
    return digits, lead, sc.sequence_encode(digits, Fs, plan, lead=lead, noise_db=12.0, seed=seed)
