"""CPU model of the spectrum bank (kq_spec_*, include/ka9q_hip.h) in float64: the same uint64 DDS phase, the same
float-rounded decimator taps and frame window as ka9q_sdr_amd/csrc/kq_spec.hip, everything else in double.

SpecModel mirrors the bank's control plane (set / remove / reset, max_rows dropping) over the whole stream it was fed;
analyzer_rows() is the math of one analyzer."""
import math

import numpy as np

GUARD, TAP_BETA = 24, 3.0
KQ_IQ_CF32, KQ_IQ_S16, KQ_IQ_S8 = 0, 1, 2


def convert(iq, gain=1.0):
    """x[n] as the bank converts it (k_spec_ingest = k_ingest, radio.c:110-122): float32 arithmetic, returned as complex128.
    complex128 input is taken as it is (an ideal stream for the model's own tests)."""
    iq = np.asarray(iq)
    g = np.float32(gain)
    if iq.dtype == np.complex128:
        return iq * float(g)
    if iq.dtype == np.complex64:
        re, im = iq.real.astype(np.float32), iq.imag.astype(np.float32)
    else:
        q = iq.reshape(-1, 2)
        sc = np.float32(1) / np.float32(32767 if iq.dtype == np.int16 else 127)
        re, im = q[:, 0].astype(np.float32) * sc, q[:, 1].astype(np.float32) * sc
    return (re * g).astype(np.float64) + 1j * (im * g).astype(np.float64)


def _i0f(x):
    """filter.c:282-293 in float32, elementwise (0.25 * x * x in double as the C expression is)"""
    x = np.asarray(x, np.float32)
    t = (0.25 * x.astype(np.float64) * x.astype(np.float64)).astype(np.float32)
    s = np.float32(1) + t
    term = t.copy()
    live = np.ones(x.shape, bool)
    for k in range(2, 40):
        nt = (term * (t / np.float32(k * k))).astype(np.float32)
        ns = (s + nt).astype(np.float32)
        term = np.where(live, nt, term)
        s = np.where(live, ns, s)
        live &= ~(term.astype(np.float64) < 1e-12 * s.astype(np.float64))
        if not live.any():
            break
    return s


def make_kaiser(M, beta):
    """filter.c:337-357 in float32: the frame window"""
    numc = np.float32(math.pi * np.float32(beta))
    inv_denom = np.float32(1.0 / float(_i0f(np.array([numc]))[0]))
    pc = np.float32(2.0 / (M - 1))
    n = np.arange(M // 2)
    p = (pc * n.astype(np.float32)).astype(np.float32) - np.float32(1)
    half = (_i0f(numc * np.sqrt((np.float32(1) - p * p).astype(np.float32))) * inv_denom).astype(np.float32)
    w = np.empty(M, np.float32)
    w[:M // 2] = half
    w[M - 1 - n] = half
    if M & 1:
        w[(M - 1) // 2] = 1
    return w


def _i0(x):
    q = 0.25 * x * x
    term, s = np.ones_like(q), np.ones_like(q)
    for k in range(1, 500):
        term = term * q / (k * k)
        s = s + term
        if np.all(term < 1e-17 * s):
            break
    return s


def design_taps(Dz):
    """Lh = 24 Dz + 1 taps: Kaiser (3.0, make_kaiser's convention) times sinc((t - 12 Dz) / Dz), sum 1; double, then float"""
    if Dz == 1:
        return np.ones(1, np.float32)
    c = GUARD * Dz // 2
    u = np.abs(np.arange(GUARD * Dz + 1) - c).astype(np.float64)
    a = math.pi * TAP_BETA
    w = _i0(a * np.sqrt(np.maximum(0.0, 1 - (u / c) ** 2))) / _i0(np.array(a))
    h = w * np.sinc(u / Dz)
    return (h / h.sum()).astype(np.float32)


def taps_power(h, Dz, Nf, B):
    """C[k] = |H(k / (Dz Nf))|^2 of the float taps for the kept bins"""
    if Dz == 1:
        return np.ones(B)
    k = np.arange(B) - B // 2
    t = np.arange(len(h))
    H = np.exp(-2j * np.pi * np.outer(k / (Dz * Nf), t)) @ h.astype(np.float64)
    return np.abs(H) ** 2


def dds_word(cycles_per_sample):
    """round(v 2^64) mod 2^64 as the C library computes it (double, round half to even)"""
    v = float(np.rint(math.ldexp(cycles_per_sample, 64)))
    return int(v) % (1 << 64)


def phase(n, s0, inc, inc2):
    """phi(n) = inc n + inc2 d (d - 1) / 2 mod 2^64, d = n - s0 (uint64 arithmetic, exact)"""
    n = np.asarray(n, np.int64)
    d = n - np.int64(s0)
    odd = (d & 1) == 1
    a = np.where(odd, d, d // 2).astype(np.uint64)
    b = np.where(odd, (d - 1) // 2, d - 1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(inc) * n.astype(np.uint64) + np.uint64(inc2) * (a * b)


def params(center=0.0, sweep=0.0, decimate=1, fft_size=1024, bins=None, hop=None, average=1, kaiser_beta=3.0):
    if bins is None:
        bins = fft_size if decimate == 1 else (3 * fft_size // 4) & ~1
    return dict(center=float(center), sweep=float(sweep), decimate=int(decimate), fft_size=int(fft_size), bins=int(bins),
                hop=int(fft_size // 2 if hop is None else hop), average=int(average), kaiser_beta=float(kaiser_beta))


def info(p, Fs):
    w = make_kaiser(p["fft_size"], p["kaiser_beta"]).astype(np.float64)
    Dz, Nf = p["decimate"], p["fft_size"]
    bw = Fs / (Dz * Nf)
    return dict(bin_bw=bw, first_bin_hz=p["center"] - p["bins"] // 2 * bw, enbw_bins=Nf * (w * w).sum() / w.sum() ** 2,
                delay_samples=12.0 * Dz if Dz > 1 else 0.0)


def counts(p, s0, n):
    """(decimated outputs, frames, rows) complete once the stream holds [0, n)"""
    last = n - 1 - s0
    P = 0 if last < 0 else last // p["decimate"] + 1
    F = 0 if P < p["fft_size"] else (P - p["fft_size"]) // p["hop"] + 1
    return P, F, F // p["average"]


def _fftconv(a, h):
    n = len(a) + len(h) - 1
    m = 1 << (n - 1).bit_length()
    return np.fft.ifft(np.fft.fft(a, m) * np.fft.fft(h.astype(np.float64), m))[:n]


def analyzer_rows(x, p, Fs, s0=0, n_end=None):
    """rows (float64 [R, B]) and their start samples of an analyzer set at stream index s0 over x[0 : n_end]"""
    n_end = len(x) if n_end is None else n_end
    Dz, Nf, B, H, K = p["decimate"], p["fft_size"], p["bins"], p["hop"], p["average"]
    P, F, R = counts(p, s0, n_end)
    if R == 0:
        return np.zeros((0, B)), np.zeros(0, np.uint64)
    inc, inc2 = dds_word(p["center"] / Fs), dds_word(p["sweep"] / (Fs * Fs))
    G = GUARD if Dz > 1 else 0
    start = s0 - G * Dz
    n = np.arange(start, s0 + (P - 1) * Dz + 1)
    xs = np.zeros(len(n), complex)
    ok = n >= 0
    xs[ok] = x[n[ok]]
    ph = phase(n, s0, inc, inc2).view(np.int64).astype(np.float64) * 2.0 ** -64
    m = xs * np.exp(-2j * np.pi * ph)
    h = design_taps(Dz)
    if Dz == 1:
        y = m[:P]
    else:
        y = _fftconv(m, h)[G * Dz + np.arange(P) * Dz]
    w = make_kaiser(Nf, p["kaiser_beta"]).astype(np.float64)
    C = taps_power(h, Dz, Nf, B)
    kept = (np.arange(B) - B // 2) % Nf
    idx = np.arange(F * 0 + R * K)[:, None] * H + np.arange(Nf)[None, :]
    X = np.fft.fft(y[idx] * w, axis=1)[:, kept]
    Pf = np.abs(X) ** 2 / w.sum() ** 2 / C
    rows = Pf.reshape(R, K, B).mean(axis=1)
    starts = (s0 + np.arange(R, dtype=np.uint64) * (K * H * Dz)).astype(np.uint64)
    return rows, starts


class SpecModel:
    """The bank's control plane over the model: analyzers set / replaced / removed between calls, rows kept up to max_rows
    (later ones dropped and counted), pulled in order."""

    def __init__(self, samprate, max_rows=64, gain_factor=1.0):
        self.Fs, self.max_rows, self.gain = samprate, max_rows, gain_factor
        self.x = np.zeros(0, complex)
        self.slots = {}   # slot -> dict(p, s0, gen, rows_seen)
        self.gen = {}
        self.ready = {}   # slot -> list of (row, start, gen)
        self.dropped = {}

    def set(self, slot, p):
        g = self.gen.get(slot, 0) + 1
        self.gen[slot] = g
        old = self.slots.get(slot)
        if old is None:
            self.ready[slot], self.dropped[slot] = [], 0
        elif old["p"]["bins"] != p["bins"]:
            self.dropped[slot] += len(self.ready[slot])
            self.ready[slot] = []
        self.slots[slot] = dict(p=dict(p), s0=len(self.x), gen=g, seen=0)

    def remove(self, slot):
        del self.slots[slot]
        self.ready[slot] = []

    def reset(self):
        self.x = np.zeros(0, complex)
        for a in self.slots.values():
            a["s0"], a["seen"] = 0, 0
        for s in self.ready:
            self.ready[s] = []

    def process(self, iq):
        self.x = np.concatenate([self.x, convert(iq, self.gain)])
        for slot, a in self.slots.items():
            rows, starts = analyzer_rows(self.x, a["p"], self.Fs, a["s0"])
            for r in range(a["seen"], len(rows)):
                if len(self.ready[slot]) < self.max_rows:
                    self.ready[slot].append((rows[r], int(starts[r]), a["gen"]))
                else:
                    self.dropped[slot] += 1
            a["seen"] = len(rows)

    def pull(self, slot, n=None):
        q = self.ready[slot]
        n = len(q) if n is None else min(n, len(q))
        out, self.ready[slot] = q[:n], q[n:]
        B = self.slots[slot]["p"]["bins"] if not out else len(out[0][0])
        return (np.array([o[0] for o in out]).reshape(-1, B), np.array([o[1] for o in out], np.uint64),
                np.array([o[2] for o in out], np.uint32))
