"""Float64 model of the rational resampler bank (include/ka9q_hip.h, kq_rsmp_*) in direct form: the prototype designed in
float64 and cast to float32 exactly as defined, every output the direct sum in float64, and beside it the sum of |g x|
that the error bound of the defined float32 fold is a multiple of."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
SCALE = F32(1.0) / F32(32767.0)


def ratio(in_rate_num, in_rate_den, out_rate):
    """P, Q: Fo in_rate_den / in_rate_num in lowest terms"""
    f = Fraction(out_rate * in_rate_den, in_rate_num)
    return f.numerator, f.denominator


def design(P, T, fi, cutoff_hz, beta):
    """g float32 [P][T]: h the Kaiser-windowed sinc of K = P T taps at rate P fi (make_kaiser's convention,
    filter.c:337-357) in float64, sum h = P; g[phi][k] = h[k P + phi]"""
    K = P * T
    m = np.arange(K, dtype=np.float64)
    pp = 2.0 * m / (K - 1) - 1.0
    w = np.i0(np.pi * beta * np.sqrt(np.maximum(0.0, 1.0 - pp * pp))) / np.i0(np.pi * beta)
    h = np.sinc(2.0 * cutoff_hz / (P * fi) * (m - (K - 1) / 2.0)) * w
    h = h * (P / h.sum())
    return np.ascontiguousarray(h.reshape(T, P).T).astype(F32)


def transition_hz(fi, T, beta):
    return 2.0 * fi * math.sqrt(1.0 + beta * beta) / T


def clean_cutoff(fi, fo, T, beta):
    return 0.5 * min(fi, fo) - 0.5 * transition_hz(fi, T, beta)


def ceil_div(a, b):
    return -(-a // b)


def count(n0, S, P, Q):
    """J of a call that brings the samples [n0, n0 + S)"""
    return ceil_div((n0 + S) * P, Q) - ceil_div(n0 * P, Q)


def bound(T):
    """forward error bound of the T-step fmaf fold as a multiple of sum |g x|, with 2 to spare"""
    return (T + 2) * 2.0 ** -24


def from_s16be(words):
    s = np.ascontiguousarray(words).view(">i2").astype(np.int16)
    return (SCALE * s.astype(F32)).astype(F32)


def scaleclip(x):
    """audio.c:22-28 on float32 samples, as int16 in host byte order (NaN: 0)"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        v = np.trunc(np.nan_to_num(F32(32767.0) * x, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)
    v = np.where(x >= 1.0, 32767, np.where(x <= -1.0, -32768, v))
    return v.astype(np.int16)


class RsmpModel:
    """One side of one slot.  feed() takes the next samples of the stream (float32 values) and returns (y, absum) float64
    for the outputs that fall into them.  start: the place on the shared grid of the first sample fed (zero before it)."""

    def __init__(self, P, Q, g, start=0):
        self.P, self.Q = P, Q
        self.g = np.asarray(g, F32).astype(np.float64)
        self.T = self.g.shape[1]
        assert self.g.shape[0] == P
        self.tail = np.zeros(self.T - 1)
        self.n = start

    def feed(self, x):
        x = np.asarray(x, F32).astype(np.float64)
        P, Q, T = self.P, self.Q, self.T
        n0, S = self.n, len(x)
        j = np.arange(ceil_div(n0 * P, Q), ceil_div((n0 + S) * P, Q), dtype=object)
        ext = np.concatenate([self.tail, x])
        self.tail = ext[len(ext) - (T - 1):]
        self.n = n0 + S
        if len(j) == 0:
            return np.zeros(0), np.zeros(0)
        nj = np.array([int(v) * Q // P - n0 for v in j], np.int64)      # place in x of each output's newest sample
        phi = np.array([int(v) * Q % P for v in j], np.int64)
        idx = nj[:, None] + (T - 1) - np.arange(T)[None, :]           # into ext
        t = self.g[phi] * ext[idx]
        return t.sum(axis=1), np.abs(t).sum(axis=1)


def resample(x, in_rate_num, in_rate_den, out_rate, T, beta, cutoff_hz=None):
    """a whole signal through the model from n = 0: float64 outputs"""
    P, Q = ratio(in_rate_num, in_rate_den, out_rate)
    fi = in_rate_num / in_rate_den
    if cutoff_hz is None:
        cutoff_hz = clean_cutoff(fi, out_rate, T, beta)
    m = RsmpModel(P, Q, design(P, T, fi, F32(cutoff_hz).astype(np.float64), F32(beta).astype(np.float64)))
    return m.feed(x)[0]
