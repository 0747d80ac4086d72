"""numpy restatement of the FSK / GMSK packet decoder bank's algorithm (include/ka9q_hip.h, kq_fsk_*) and a test-signal
generator.  The filter and the threshold are vectorised int64; bit clock, descrambler, NRZI and deframer are a plain loop.
Everything after the quantiser is integer arithmetic, so the bank must give the model's records bit for bit."""
import numpy as np

from common import afsk_bits

MASK17 = 0x1FFFF


def design_taps(K, cutoff_hz, Fs, beta):
    """hq: Kaiser-windowed sinc in float64 (make_kaiser's convention, filter.c:337-357), sum 1, times 32768, rounded"""
    k = np.arange(K, dtype=np.float64)
    pp = 2.0 * k / (K - 1) - 1.0
    w = np.i0(np.pi * beta * np.sqrt(np.maximum(0.0, 1.0 - pp * pp))) / np.i0(np.pi * beta)
    h = np.sinc(2.0 * cutoff_hz / Fs * (k - (K - 1) / 2.0)) * w
    return np.rint(h / h.sum() * 32768.0).astype(np.int64)


def quantise(x, scale, s16=False):
    """q: float32 multiply, round to nearest even, clamp; NaN reads as 0.  s16: int16 words taken as they are"""
    if s16:
        return np.maximum(np.asarray(x).astype(np.int64), -32767)
    v = np.rint(np.asarray(x, np.float32) * np.float32(scale))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, -32767, 32767).astype(np.int64)


def running(y, W, op):
    """op over y[i - W + 1 .. i] for i >= W - 1, by doubling"""
    m = y.copy()
    span = 1
    while 2 * span <= W:
        m[span:] = op(m[span:], m[:-span])
        span *= 2
    off = W - span
    return op(m[W - 1:], m[W - 1 - off:len(m) - off])


def crc_x25(data):
    crc = 0xFFFF
    for byte in data:
        for i in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ (byte >> i)) & 1 else 0)
    return crc


class FskModel:
    """One slot.  feed() takes the next samples of the stream; frames, counters and the status fields are the bank's."""

    def __init__(self, Fs, baud, K, scrambled=True, cutoff_hz=None, beta=2.0, window_bits=16.0, input_scale=4096.0, pll_shift=3,
                 max_frames=16, max_frame_bytes=512, min_bytes=8, taps=None, start=0):
        self.K, self.W = K, int(np.rint(np.float32(window_bits).astype(np.float64) * Fs / baud))
        self.hq = np.asarray(taps, np.int64) if taps is not None else design_taps(K, 0.6 * baud if cutoff_hz is None else cutoff_hz,
                                                                                   Fs, beta)
        assert len(self.hq) == K and np.abs(self.hq).sum() <= 65535
        self.inc = int(np.rint(2.0 ** 32 * baud / Fs))
        self.scale, self.shift, self.scrambled = input_scale, pll_shift, bool(scrambled)
        self.max_frames, self.mfb, self.min_bytes = max_frames, max_frame_bytes, min_bytes
        self.H = K - 1 + self.W - 1
        self.q = np.zeros(self.H, np.int64)      # the carried inputs
        self.n = start                           # the next sample's place on the grid
        self.s = self.sr = self.dprev = self.uprev = 0
        self.ones = self.in_frame = self.nbits = 0
        self.buf = bytearray(self.mfb)
        self.bits = self.frames_good = self.frames_bad = self.aborts = self.dropped = 0
        self.level = 0
        self.frames = []                         # the arena: (bytes, end_sample, end_bit)

    def clear_frames(self):
        self.frames = []

    def front(self, x, s16=False):
        """d of the new samples"""
        q = np.concatenate([self.q, quantise(x, self.scale, s16)])
        n = len(q) - self.H
        y = np.convolve(q, self.hq)[self.K - 1:len(q)]          # y of q[K - 1:], all its taps inside q
        top, bot = running(y, self.W, np.maximum), running(y, self.W, np.minimum)
        assert len(top) == n
        d = (2 * y[self.W - 1:] > top + bot).astype(np.int64)
        self.level = int(top[-1] - bot[-1])
        self.q = q[n:]
        return d

    def feed(self, x, s16=False):
        if len(x) == 0:
            return
        d = self.front(x, s16)
        for dn in d.tolist():
            if dn != self.dprev:
                self.s -= self.s >> self.shift
            self.dprev = dn
            t = self.s + self.inc
            if t >= 1 << 31:
                self.s = t - (1 << 32)
                self._channel_bit(dn)
            else:
                self.s = t
            self.n += 1

    def _channel_bit(self, c):
        self.bits += 1
        u = c
        if self.scrambled:
            u = c ^ ((self.sr >> 16) & 1) ^ ((self.sr >> 11) & 1)
            self.sr = ((self.sr << 1) | c) & MASK17
        b = int(u == self.uprev)
        self.uprev = u
        if b:
            self.ones = min(self.ones + 1, 7)
            if self.ones == 7:
                self.aborts += self.in_frame
                self.in_frame = 0
            elif self.in_frame:
                self._append(1)
            return
        if self.ones == 6:
            nb = self.nbits - 7
            if self.in_frame and nb >= 8 * self.min_bytes:
                if nb % 8 == 0 and nb // 8 <= self.mfb and crc_x25(self.buf[:nb // 8]) == 0xf0b8:
                    self.frames_good += 1
                    if len(self.frames) < self.max_frames:
                        self.frames.append((bytes(self.buf[:nb // 8]), self.n, self.bits))
                    else:
                        self.dropped += 1
                else:
                    self.frames_bad += 1
            self.in_frame, self.nbits = 1, 0
            self.buf = bytearray(self.mfb)
        elif self.ones < 5 and self.in_frame:
            self._append(0)
        self.ones = 0

    def _append(self, bit):
        if self.nbits < 8 * self.mfb:
            self.buf[self.nbits >> 3] |= bit << (self.nbits & 7)
        self.nbits = min(self.nbits + 1, (1 << 31) - 1)

    def status(self):
        return dict(bits=self.bits, frames_good=self.frames_good, frames_bad=self.frames_bad, aborts=self.aborts,
                    dropped=self.dropped, pll_phase=self.s, in_frame=self.in_frame, level=self.level)


# ---- generator ----
def scramble(u):
    """G3RUH scrambler, 1 + x^12 + x^17: the inverse of the decoder's step"""
    sr, out = 0, []
    for b in u:
        c = b ^ ((sr >> 16) & 1) ^ ((sr >> 11) & 1)
        sr = ((sr << 1) | c) & MASK17
        out.append(c)
    return out


def descramble(c_bits):
    sr, out = 0, []
    for c in c_bits:
        out.append(c ^ ((sr >> 16) & 1) ^ ((sr >> 11) & 1))
        sr = ((sr << 1) | c) & MASK17
    return out


def line_bits(data_bits, scrambled):
    """HDLC data bits -> NRZI (a 0 toggles) -> scrambler: the channel bits"""
    u, cur = [], 0
    for b in data_bits:
        if b == 0:
            cur ^= 1
        u.append(cur)
    return scramble(u) if scrambled else u


def shape(chan_bits, Fs, baud, ppm=0.0, bt=0.5):
    """rectangular +-1 symbols at Fs / baud (1 + ppm 1e-6) samples per bit through a Gaussian pulse of that BT; float64"""
    spb = Fs / baud * (1.0 + ppm * 1e-6)
    n = int(len(chan_bits) * spb)
    lv = 2.0 * np.asarray(chan_bits, np.float64) - 1.0
    rect = lv[np.minimum((np.arange(n) / spb).astype(np.int64), len(chan_bits) - 1)]
    sigma = np.sqrt(np.log(2.0)) / (2.0 * np.pi * bt) * spb
    half = int(np.ceil(3.0 * spb))
    g = np.exp(-0.5 * (np.arange(-half, half + 1) / sigma) ** 2)
    return np.convolve(rect, g / g.sum(), mode="same")


def fsk_signal(frames, Fs, baud, scrambled=True, ppm=0.0, amp=0.3, dc=0.0, noise=0.0, seed=0, lead=0.01, tail=0.01,
               lead_flags=8, gap_flags=3, preamble=False):
    """a burst: `lead` seconds of silence, (AIS: the 24-bit alternating preamble,) flags, the frames, flags, `tail` seconds
    of silence; plus dc and white noise all along.  float32, in the units of the decoder's input (rad/sample)"""
    bits = afsk_bits(frames, lead_flags=lead_flags, gap_flags=gap_flags)
    if preamble:
        bits = [0] * 24 + bits                      # NRZI turns zeros into alternating line bits
    sig = amp * shape(line_bits(bits, scrambled), Fs, baud, ppm)
    x = np.concatenate([np.zeros(int(lead * Fs)), sig, np.zeros(int(tail * Fs))]) + dc
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(len(x))
    return x.astype(np.float32)


def make_frames(count, seed, lo=12, hi=40):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8)) for _ in range(count)]
