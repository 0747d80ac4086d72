"""Float64 model of the RDS decoder (include/ka9q_hip.h, kq_rds_*), in numpy direct form: the matched response designed by
window_filter's procedure in float64, the 57 kHz baseband by direct convolution with its taps (taken at every Dr-th
sample, one np.convolve per polyphase branch: no frames in the filter), the per-frame carrier and bit-clock tracker, the
bit sampler, the differential decoder and the block / group machine.  Also the generator: groups -> 26-bit blocks ->
differential -> shaped biphase pulse train on a 57 kHz subcarrier, added to a wfm_model multiplex.  Parameters that the C
side keeps as float are rounded to float32 first, as it sees them."""
import math

import numpy as np

import wfm_model as wm

SUB_HZ, BIT_HZ = 57000, 1187.5
LEAD = 4.0                                      # bit periods from the generator's first sample to bit 0's centre
POLY = 0x5B9                                    # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
POSITION = {"A": 0, "B": 1, "C": 2, "C'": 2, "D": 3}
_BY_SYNDROME = {v: k for k, v in OFFSETS.items()}


def crc10(w):
    """remainder of w x^10 modulo the generator, w of 16 bits"""
    r = (w & 0xFFFF) << 10
    for b in range(25, 9, -1):
        if (r >> b) & 1:
            r ^= POLY << (b - 10)
    return r & 0x3FF


def block(info, name):
    """the 26-bit word of a 16-bit information word with offset `name`"""
    return ((info & 0xFFFF) << 10) | (crc10(info) ^ OFFSETS[name])


def hit(word):
    """the offset name whose syndrome the 26-bit word has, or None"""
    return _BY_SYNDROME.get(crc10(word >> 10) ^ (word & 0x3FF))


def group_bits(groups):
    """groups: (b0, b1, b2, b3) or (b0, b1, b2, b3, version_b) -> the data bits, most significant first"""
    out = []
    for g in groups:
        names = ["A", "B", "C'" if len(g) > 4 and g[4] else "C", "D"]
        for w, nm in zip(g[:4], names):
            v = block(w, nm)
            out.extend((v >> (25 - k)) & 1 for k in range(26))
    return np.array(out, np.int64)


def _shaped(u):
    """the cosine-shaped pulse of IEC 62106 (response cos(pi f t_d / 4) for |f| <= 2 / t_d) at u = t / t_d"""
    return np.sinc(0.5 + 4 * u) + np.sinc(0.5 - 4 * u)


def _symbol(u):
    """the biphase symbol _shaped(u) - _shaped(u - 1/2) with one cosine: _shaped(u) = cos(4 pi u) / (pi (1/4 - 16 u^2)), and
    cos(4 pi (u - 1/2)) = cos(4 pi u)"""
    v = u - 0.5
    d0, d1 = 0.25 - 16 * u * u, 0.25 - 16 * v * v
    near = (np.abs(d0) < 1e-6) | (np.abs(d1) < 1e-6)      # the removable singularities at u = +-1/8, 3/8, 5/8
    d0, d1 = np.where(near, 1.0, d0), np.where(near, 1.0, d1)
    p = np.cos(4 * np.pi * u) / np.pi * (1.0 / d0 - 1.0 / d1)
    if near.any():
        p[near] = _shaped(u[near]) - _shaped(v[near])
    return p


def biphase(bits, n, Fc, eps=0.0, lead=LEAD, span=8):
    """the shaped biphase baseband of the data bits at n samples of rate Fc, peak 1; the transmitter's clock runs fast by
    eps (bit rate 1187.5 (1 + eps)); bit i is centred (i + lead) bit periods in.  Each pulse is kept for +-span bits."""
    c = np.cumsum(bits) & 1                     # differential: c_i = c_{i-1} xor b_i
    amp = 1.0 - 2.0 * c
    spb = Fc / (BIT_HZ * (1.0 + eps))
    s = np.zeros(n)
    w = int(span * spb) + 1
    off = np.arange(-w, w + 1)
    for i, a in enumerate(amp):
        ctr = (i + lead) * spb
        idx = int(ctr) + off
        ok = (idx >= 0) & (idx < n)
        u = (idx[ok] - ctr) / spb
        s[idx[ok]] += a * _symbol(u)
    return s / np.max(np.abs(s))


def settle_bits(Fc, M, keyed=None):
    """the decoder's first bits lie in the filter's fill-in, where z is the window's leading edge and |y| is near 0: the
    count of bits until the centre tap of the M-tap filter has reached the first keyed sample, `keyed` samples after the
    start of the slot's first frame (by default bit 0's centre in a composite of this generator)"""
    keyed = LEAD * Fc / BIT_HZ if keyed is None else keyed
    return math.ceil((keyed + (M - 1) / 2) * BIT_HZ / Fc)


def settle_frames(Fc, L, M, keyed=None):
    """the frames that end before, or hold, that same instant: in them z is partly or wholly the filter's fill-in"""
    keyed = LEAD * Fc / BIT_HZ if keyed is None else keyed
    return math.ceil((keyed + (M - 1) / 2) / L)


def parts(n, Fc, bits, eps=0.0, pilot=0.1, seed=0, program=True, deviation_hz=75000.0):
    """the slow parts of a composite: (stereo programme and pilot by wm.multiplex in rad/sample, the shaped biphase train of
    `bits` times cos and times sin of the 57 kHz (1 + eps) carrier at full deviation)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / Fc
    if program:
        lt = rng.uniform(0.1, 0.5) * np.sin(2 * np.pi * rng.uniform(200, 14000) * t)
        rt = rng.uniform(0.1, 0.5) * np.sin(2 * np.pi * rng.uniform(200, 14000) * t)
    else:
        lt = rt = 0.0
    x = wm.multiplex(n, Fc, lt, rt, pilot=pilot, pilot_hz=wm.PILOT_HZ * (1 + eps), deviation_hz=deviation_hz,
                     phase=rng.uniform(0, 6))
    w = biphase(bits, n, Fc, eps) * (2 * np.pi * deviation_hz / Fc)
    a = 2 * np.pi * SUB_HZ * (1 + eps) * t
    return x, w * np.cos(a), w * np.sin(a)


def combine(p, injection=0.035, theta=0.0, noise=0.01, seed=0):
    """programme + the subcarrier at `injection` of the peak deviation and phase theta + white noise of `noise` rad/sample"""
    x, wc, ws = p
    rng = np.random.default_rng(seed)
    return x + injection * (math.cos(theta) * wc - math.sin(theta) * ws) + noise * rng.standard_normal(len(x))


def composite(n, Fc, bits, injection=0.035, eps=0.0, theta=0.0, pilot=0.1, noise=0.01, seed=0, program=True,
              deviation_hz=75000.0):
    """a broadcast composite in rad/sample with RDS, sample-clock error eps (the transmitter's clock runs fast by eps)"""
    return combine(parts(n, Fc, bits, eps, pilot, seed, program, deviation_hz), injection, theta, noise, seed + 1)


class Machine:
    """bits -> blocks -> groups (the header's "Blocks", "Unsynced", "Synced")"""

    def __init__(self, lose_after=10):
        self.lose_after = lose_after
        self.reg = self.nbits = 0
        self.synced = self.expect = self.next_at = self.bad = 0
        self.rem = None                          # (bit count, position, info, is C')
        self.ok_count = self.bad_count = 0
        self.groups = []                         # (block[4], ok, version_b, bit)
        self._open()

    def _open(self):
        self.blk, self.ok, self.vb = [0, 0, 0, 0], 0, 0

    def _put(self, pos, info, cp):
        self.blk[pos] = info
        self.ok |= 1 << pos
        self.vb |= int(cp)
        self.ok_count += 1

    def _emit(self):
        self.groups.append((tuple(self.blk), self.ok, self.vb, self.nbits))
        self._open()

    def push(self, b):
        self.nbits += 1
        self.reg = ((self.reg << 1) | int(b)) & 0x3FFFFFF
        if self.nbits < 26:
            return
        name = hit(self.reg)
        info = self.reg >> 10
        if not self.synced:
            if name is None:
                return
            pos, cp = POSITION[name], name == "C'"
            if self.rem and self.nbits == self.rem[0] + 26 and pos == (self.rem[1] + 1) % 4:
                self._open()
                if pos > 0:
                    self._put(self.rem[1], self.rem[2], self.rem[3])
                self._put(pos, info, cp)
                if pos == 3:
                    self._emit()
                self.synced, self.expect, self.next_at, self.bad = 1, (pos + 1) % 4, self.nbits + 26, 0
            self.rem = (self.nbits, pos, info, cp)
            return
        if self.nbits != self.next_at:
            return
        pos = self.expect
        self.blk[pos] = info
        if name is not None and POSITION[name] == pos:
            self.ok |= 1 << pos
            self.vb |= int(name == "C'")
            self.ok_count += 1
            self.bad = 0
        else:
            self.bad += 1
            self.bad_count += 1
        if pos == 3:
            self._emit()
        self.expect, self.next_at = (pos + 1) % 4, self.next_at + 26
        if self.bad >= self.lose_after:
            self.synced, self.rem = 0, None
            self._open()


def decode_bits(bits, lose_after=10):
    m = Machine(lose_after)
    for b in bits:
        m.push(b)
    return m


class RdsModel:
    def __init__(self, comp_rate, decimate, L, M, kaiser_beta=3.0):
        self.Fc, self.Dr, self.L, self.M = int(comp_rate), int(decimate), L, M
        self.N, self.Lr, self.Fr = L + M - 1, L // decimate, int(comp_rate) // decimate
        self.spb = self.Fr / BIT_HZ
        self.beta = wm.f32(kaiser_beta)
        g = wm.bins_hz(self.N, float(self.Fc)) - SUB_HZ
        td = 1.0 / BIT_HZ
        R = np.where(np.abs(g) <= 2.0 / td, -1j * np.sin(np.pi * g * td / 2) * np.cos(np.pi * g * td / 4), 0.0)
        self.h = wm.window_taps(R, M, self.beta)

    def baseband(self, x):
        """z[k] = (h * x)[k Dr] exp(-j 2 pi 57000 k Dr / Fc) for the k of the completed frames"""
        x = np.asarray(x, np.float64)
        Dr = self.Dr
        K = (len(x) // self.L) * self.Lr
        y = np.zeros(K, np.complex128)
        for p in range(Dr):                      # y[k Dr] = sum_q h[q Dr + p] x[(k - q) Dr - p]
            hp = self.h[p::Dr]
            idx = np.arange(K) * Dr - p
            xp = np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)
            y += np.convolve(xp, hp.real)[:K] + 1j * np.convolve(xp, hp.imag)[:K]
        k = np.arange(K, dtype=np.int64)
        return y * np.exp(-2j * np.pi * ((SUB_HZ * k * Dr) % self.Fc) / self.Fc)

    def decode(self, x, start=0, track_ms=20.0, lose_after=10):
        """x: the composite from stream index 0, zero before `start` (where the slot was set).  -> dict: z [F Lr]; per
        frame phase, timing, level, synced, blocks_ok, blocks_bad [F] (zero before the slot's first frame); bits, soft
        (y_i); groups [(block[4], ok, version_b, bit)] and group_frame (the frame each was emitted in)"""
        L, Lr, Fr, spb = self.L, self.Lr, self.Fr, self.spb
        z = self.baseband(x)
        F = len(z) // Lr
        fs = start // L
        alpha = 1.0 - math.exp(-L / (self.Fc * wm.f32(track_ms) * 1e-3))
        A = B = 0j
        phi = tau = 0.0
        i = None
        cprev = 0
        m = Machine(lose_after)
        st = {k: np.zeros(F) for k in ("phase", "timing", "level")}
        st.update({k: np.zeros(F, np.int64) for k in ("synced", "blocks_ok", "blocks_bad")})
        bits, soft, gframe = [], [], []
        for f in range(fs, F):
            zz = z[f * Lr:(f + 1) * Lr]
            k = np.arange(f * Lr, (f + 1) * Lr, dtype=np.int64)
            p2 = np.abs(zz) ** 2
            S, P = np.sum(zz * zz), np.sum(p2)
            E = np.sum(p2 * np.exp(-2j * np.pi * ((2375 * k) % (2 * Fr)) / (2 * Fr)))
            A += alpha * (S - A)
            B += alpha * (E - B)
            w = np.angle(A) - 2 * phi
            phi += 0.5 * (w - 2 * np.pi * np.rint(w / (2 * np.pi)))
            phi -= 2 * np.pi * math.ceil((phi - np.pi) / (2 * np.pi))      # into (-pi, pi]
            u = -np.angle(B) / (2 * np.pi) - tau
            tau += u - np.rint(u)
            if i is None:                        # the least i with t_i >= fs Lr
                i = math.ceil(f * Lr / spb - tau)
                while (i + tau) * spb < f * Lr:
                    i += 1
                while (i - 1 + tau) * spb >= f * Lr:
                    i -= 1
            rot = np.exp(-1j * phi)
            while True:
                t = (i + tau) * spb
                if not t + 1 < (f + 1) * Lr:
                    break
                k0 = math.floor(t)
                r = t - k0
                z0 = z[k0] if k0 >= 0 else 0.0
                z1 = z[k0 + 1] if k0 + 1 >= 0 else 0.0
                yv = ((z0 + r * (z1 - z0)) * rot).real
                c = int(yv < 0)
                bits.append(c ^ cprev)
                soft.append(yv)
                cprev = c
                before = len(m.groups)
                m.push(bits[-1])
                gframe.extend([f] * (len(m.groups) - before))
                i += 1
            st["phase"][f], st["timing"][f], st["level"][f] = phi, tau, math.sqrt(P / Lr)
            st["synced"][f], st["blocks_ok"][f], st["blocks_bad"][f] = m.synced, m.ok_count, m.bad_count
        st.update(z=z, bits=np.array(bits, np.int64), soft=np.array(soft), groups=m.groups,
                  group_frame=np.array(gframe, np.int64))
        return st
