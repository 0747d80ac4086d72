"""Float64 model of the monitor mixer bank (include/ka9q_hip.h, kq_mon_*) in direct form: gains and the PCM scaling in
float32 exactly as defined, the sum over a bus's members in float64, and beside every output sample the sum of |g x| that
the error bound of the defined float32 summation is a multiple of."""
import math

import numpy as np

F32 = np.float32
SCALE = F32(1.0) / F32(32767.0)          # monitor.c:88


def c_round(x):
    """C's round() of a non-negative double: halves go up"""
    r = math.floor(x)
    return int(r + 1 if x - r >= 0.5 else r)


def history(samprate):
    return c_round(0.001 * samprate)


def gains(gain, pan):
    """monitor.c:440-441 in float"""
    g, p = F32(gain), F32(pan)
    return g * (F32(1) - p) / F32(2), g * (F32(1) + p) / F32(2)


def delays(pan, samprate):
    """monitor.c:444-447: the float pan times .001 times the rate in double, rounded"""
    p = float(F32(pan))
    dl = c_round(p * .001 * samprate) if p > 0 else 0
    dr = c_round(-p * .001 * samprate) if p < 0 else 0
    return dl, dr


def from_s16be(words):
    """network-order int16 words (an array of dtype ">i2", or the raw words in any other 2-byte dtype) as the float
    samples of monitor.c:492"""
    s = np.ascontiguousarray(words).view(">i2").astype(np.int16)
    return (SCALE * s.astype(F32)).astype(F32)


def to_s16be(x):
    """float samples in [-1, 1] as network-order words, rounded to nearest"""
    return np.rint(np.asarray(x, np.float64) * 32767).astype(">i2")


def scaleclip(x):
    """audio.c:22-28 on float32 samples, as int16 in host byte order (NaN: 0)"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        v = np.trunc(np.nan_to_num(F32(32767.0) * x, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)
    v = np.where(x >= 1.0, 32767, np.where(x <= -1.0, -32768, v))
    return v.astype(np.int16)


def bound(K):
    """forward error bound of the defined summation as a multiple of sum |g x|: a chunk's fold of min(K, 64) fmaf, ceil(K / 64)
    additions of partials, and 2 to spare"""
    return (min(K, 64) + -(-K // 64) + 2) * 2.0 ** -24


class MonModel:
    def __init__(self, samprate, max_buses):
        self.samprate, self.max_buses, self.H = samprate, max_buses, history(samprate)
        self.s = {}

    def set(self, slot, source=0, bus=0, channels=1, gain=1.0, pan=0.0, muted=0):
        self.s[slot] = dict(source=source, bus=bus, channels=channels, gain=gain, pan=pan, muted=bool(muted),
                            tail=np.zeros((self.H, 2)))

    def adjust(self, slot, gain, pan, muted=0):
        self.s[slot].update(gain=gain, pan=pan, muted=bool(muted))

    def remove(self, slot):
        del self.s[slot]

    def reset(self):
        for v in self.s.values():
            v["tail"] = np.zeros((self.H, 2))

    def samples(self, audio, v, block_len, nblocks, row_stride):
        """the session's frames of the call, float64 [T][2]"""
        ch = v["channels"]
        row = audio[v["source"]]
        row = from_s16be(row) if row.dtype.itemsize == 2 else row.astype(F32)
        x = np.concatenate([row[k * row_stride:k * row_stride + ch * block_len] for k in range(nblocks)])
        x = x.astype(np.float64).reshape(-1, ch)
        return np.repeat(x, 2, axis=1) if ch == 1 else x

    def process(self, audio, block_len, nblocks=1, row_stride=None):
        """audio [rows][W], float32 or network-order int16 words.  Returns out, absum float64 [max_buses][T][2] and
        sessions, active int [max_buses]"""
        audio = np.asarray(audio)
        if row_stride is None:
            row_stride = audio.shape[1] // nblocks
        T, H = block_len * nblocks, self.H
        out = np.zeros((self.max_buses, T, 2))
        absum = np.zeros((self.max_buses, T, 2))
        sessions = np.zeros(self.max_buses, int)
        active = np.zeros(self.max_buses, int)
        for slot in sorted(self.s):
            v = self.s[slot]
            x = self.samples(audio, v, block_len, nblocks, row_stride)
            ext = np.concatenate([v["tail"], x])
            v["tail"] = ext[-H:] if H else ext[:0]
            if v["muted"]:
                continue
            b = v["bus"]
            sessions[b] += 1
            active[b] += bool(np.any(x != 0))
            for side, g, d in zip((0, 1), gains(v["gain"], v["pan"]), delays(v["pan"], self.samprate)):
                t = float(g) * ext[H - d:H - d + T, side]
                out[b, :, side] += t
                absum[b, :, side] += np.abs(t)
        return out, absum, sessions, active
