"""Two numpy models of the raw A/D conditioning stage (kq_fe_*, include/ka9q_hip.h).

exact    the definition the library implements: per block the exact integer moments and the recursion in float64,
         per sample the reference's unfused float32 arithmetic.  Bit for bit what the GPU must give, however the
         stream is cut into calls.
literal  the reference's own loop (hackrf.c:122-196 for int8, funcube.c:287-390 for int16) with its C promotions and
         its sequential float32 sums, one block per upcall.  np.cumsum(..., dtype=float32)[-1] is a sequential sum.
"""
import numpy as np

S8, S16 = 0, 1
F = np.float32
STATUS_FIELDS = ("samples", "blocks", "clips", "DC_i", "DC_q", "imbalance", "sinphi", "in_power", "gain_i", "gain_q",
                 "secphi", "tanphi")


def scale_of(fmt):
    return F(1. / 32767.) if fmt == S16 else F(1. / 127.)   # a double quotient stored in a float (hackrf.c:78)


def to_s16(v):
    """funcube.c:348 round(v * SHRT_MAX): C's round (half away from zero), saturated."""
    r = (np.asarray(v, F) * F(32767)).astype(np.float64)
    r = np.sign(r) * np.floor(np.abs(r) + 0.5)
    return np.clip(r, -32768, 32767).astype(np.int16)


def _ints(raw, fmt):
    """raw [n, 2] -> int64 I, Q with the int8 rule applied (hackrf.c:146-153), and the number of clips"""
    raw = np.asarray(raw)
    i, q = raw[:, 0].astype(np.int64), raw[:, 1].astype(np.int64)
    clips = 0
    if fmt == S8:
        clips = int(np.count_nonzero(i == -128) + np.count_nonzero(q == -128))
        i, q = np.maximum(i, -127), np.maximum(q, -127)
    return i, q, clips


def _condition(i, q, fmt, st):
    sc = scale_of(fmt)
    x = i.astype(F) * sc - st["DC_i"]
    y = q.astype(F) * sc - st["DC_q"]
    x = x * st["gain_i"]
    y = y * st["gain_q"]
    y = st["secphi"] * y - st["tanphi"] * x
    return x, y


def _initial():
    return dict(samples=0, blocks=0, clips=0, DC_i=F(0), DC_q=F(0), imbalance=F(1), sinphi=F(0), in_power=F(0),
                gain_i=F(1), gain_q=F(1), secphi=F(1), tanphi=F(0))


class Exact:
    """The definition, with the open block's moments carried across calls."""

    def __init__(self, fmt, block, adc_samprate, dc_alpha, power_alpha=1.0):
        self.fmt, self.block = fmt, int(block)
        self.dc_alpha = np.float64(dc_alpha)
        self.rate = np.float64(block) / (np.float64(adc_samprate) * np.float64(power_alpha))
        self.reset()

    def reset(self):
        self.st = _initial()
        self.filled = 0
        self.mom = [0, 0, 0, 0, 0]   # Python integers: exact
        self.open_clips = 0

    def _update(self):
        st, D = self.st, np.float64
        S, n = D(scale_of(self.fmt)), D(self.block)
        SS = S * S
        SI, SQ, SII, SQQ, SIQ = (D(m) for m in self.mom)   # below 2^53: exact
        DC_i, DC_q, gain_i, gain_q = D(st["DC_i"]), D(st["DC_q"]), D(st["gain_i"]), D(st["gain_q"])
        sI, sQ = S * SI, S * SQ
        i_energy = SS * SII - D(2.0) * DC_i * sI + n * (DC_i * DC_i)
        q_energy = SS * SQQ - D(2.0) * DC_q * sQ + n * (DC_q * DC_q)
        cross = SS * SIQ - DC_q * sI - DC_i * sQ + n * (DC_i * DC_q)
        dotprod = (gain_i * gain_q) * cross
        st["DC_i"] = F(DC_i + self.dc_alpha * (sI - n * DC_i))
        st["DC_q"] = F(DC_q + self.dc_alpha * (sQ - n * DC_q))
        block_energy = D(0.5) * (i_energy + q_energy)
        if block_energy > 0:
            with np.errstate(all="ignore"):
                st["in_power"] = F(block_energy / n)
                imbalance, sinphi = D(st["imbalance"]), D(st["sinphi"])
                st["imbalance"] = F(imbalance + self.rate * (i_energy / q_energy - imbalance))
                dpn = dotprod / block_energy
                st["sinphi"] = F(sinphi + self.rate * (dpn - sinphi))
                imbalance, sinphi = D(st["imbalance"]), D(st["sinphi"])
                st["gain_q"] = F(np.sqrt(D(0.5) * (D(1.0) + imbalance)))
                st["gain_i"] = F(np.sqrt(D(0.5) * (D(1.0) + D(1.0) / imbalance)))
                st["secphi"] = F(D(1.0) / np.sqrt(D(1.0) - sinphi * sinphi))
                st["tanphi"] = F(D(st["sinphi"]) * D(st["secphi"]))
        st["samples"] += self.block
        st["blocks"] += 1
        st["clips"] += self.open_clips
        self.mom = [0, 0, 0, 0, 0]
        self.open_clips = 0
        self.filled = 0

    def process(self, raw):
        """raw [n, 2] -> (complex64[n], int16[n, 2], [status after each block completed in the call])"""
        i, q, _ = _ints(raw, self.fmt)
        n = len(i)
        out = np.empty(n, np.complex64)
        statuses = []
        pos = 0
        while pos < n:
            take = min(self.block - self.filled, n - pos)
            si, sq = i[pos:pos + take], q[pos:pos + take]
            x, y = _condition(si, sq, self.fmt, self.st)
            out.real[pos:pos + take] = x
            out.imag[pos:pos + take] = y
            for k, v in enumerate((si.sum(), sq.sum(), (si * si).sum(), (sq * sq).sum(), (si * sq).sum())):
                self.mom[k] += int(v)
            self.open_clips += _ints(np.asarray(raw)[pos:pos + take], self.fmt)[2]
            self.filled += take
            pos += take
            if self.filled == self.block:
                self._update()
                statuses.append(dict(self.st))
        s16 = np.stack([to_s16(out.real), to_s16(out.imag)], axis=1)
        return out, s16, statuses


def exact(raw, fmt, block, adc_samprate, dc_alpha, power_alpha=1.0):
    return Exact(fmt, block, adc_samprate, dc_alpha, power_alpha).process(raw)


def _seq(v):
    """sequential float32 sum, as a C loop forms it"""
    return np.cumsum(v, dtype=F)[-1] if len(v) else F(0)


def literal(raw, fmt, block, adc_samprate, dc_alpha, power_alpha=1.0):
    """The reference's loop, one upcall per full block (a ragged end is conditioned but never updates).
    -> (complex64[n], [status after each block])"""
    D = np.float64
    i, q, _ = _ints(raw, fmt)
    n = len(i)
    sc = scale_of(fmt)
    st = _initial()
    DC_alpha, Power_alpha = F(dc_alpha), F(power_alpha)
    samprate = int(adc_samprate)
    if fmt == S8:   # hackrf.c:138: float rate_factor = 1./(ADC_samprate * Power_alpha), used as rate_factor * samples
        rate_factor = F(D(1.) / D(F(samprate) * Power_alpha))
        rate = rate_factor * F(block)
    else:           # funcube.c:297: float rate_factor = Blocksize/(ADC_samprate * Power_alpha)
        rate = F(block) / (F(samprate) * Power_alpha)
    out = np.empty(n, np.complex64)
    statuses = []
    for pos in range(0, n, block):
        ri, rq = raw[pos:pos + block, 0], raw[pos:pos + block, 1]
        si, sq = i[pos:pos + block], q[pos:pos + block]
        re, im = si.astype(F) * sc, sq.astype(F) * sc
        sum_i, sum_q = _seq(re), _seq(im)
        re, im = re - st["DC_i"], im - st["DC_q"]
        i_energy, q_energy = _seq(re * re), _seq(im * im)
        re, im = re * st["gain_i"], im * st["gain_q"]
        dotprod = _seq(re * im)
        im = st["secphi"] * im - st["tanphi"] * re
        out.real[pos:pos + block], out.imag[pos:pos + block] = re, im
        if len(si) < block:
            break
        samples = F(block)
        with np.errstate(all="ignore"):
            st["DC_i"] = F(st["DC_i"] + DC_alpha * (sum_i - samples * st["DC_i"]))
            st["DC_q"] = F(st["DC_q"] + DC_alpha * (sum_q - samples * st["DC_q"]))
            block_energy = F(D(0.5) * D(F(i_energy + q_energy)))
            if block_energy > 0:
                st["in_power"] = F(block_energy / samples)
                st["imbalance"] = F(st["imbalance"] + rate * (F(i_energy / q_energy) - st["imbalance"]))
                dpn = F(dotprod / block_energy)
                st["sinphi"] = F(st["sinphi"] + rate * (dpn - st["sinphi"]))
                st["gain_q"] = np.sqrt(F(D(0.5) * D(F(1) + st["imbalance"])))
                st["gain_i"] = np.sqrt(F(D(0.5) * (D(1) + D(1.) / D(st["imbalance"]))))
                st["secphi"] = F(1) / np.sqrt(F(F(1) - st["sinphi"] * st["sinphi"]))
                st["tanphi"] = F(st["sinphi"] * st["secphi"])
        st["samples"] += block
        st["blocks"] += 1
        if fmt == S8:
            st["clips"] += int(np.count_nonzero(ri == -128) + np.count_nonzero(rq == -128))
        statuses.append(dict(st))
    return out, statuses


def make_raw(fmt, n, seed, tone=0.3, noise=0.05, dc=(0.02, -0.03), gain_q=1.1, phase=0.05, cycles_per=64.0):
    """A/D samples of a tone plus noise through a front end with DC offset, Q gain error and phase error, as
    integers of the format, [n, 2]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    w = 2 * np.pi / cycles_per
    i = tone * np.cos(w * t) + noise * rng.standard_normal(n) + dc[0]
    q = gain_q * (tone * np.sin(w * t + phase) + noise * rng.standard_normal(n)) + dc[1]
    full = 32767 if fmt == S16 else 127
    lim = (-32768, 32767) if fmt == S16 else (-128, 127)
    out = np.stack([np.clip(np.round(i * full), *lim), np.clip(np.round(q * full), *lim)], axis=1)
    return out.astype(np.int16 if fmt == S16 else np.int8)
