"""Float64 model of the wideband FM stereo decoder (include/ka9q_hip.h, kq_wfm_*), in numpy direct form: the two responses
designed by window_filter's procedure in float64, the pilot, difference, sum and output signals by direct convolution with
their taps, and the per-frame pilot status with the flag's hysteresis.  Parameters that the C side keeps as float are
rounded to float32 first, as it sees them."""
import numpy as np

PILOT_HZ, AUDIO_HZ = 19000.0, 15000.0


def f32(v):
    return float(np.float32(v))


def kaiser(M, beta):
    """make_kaiser(M, beta) (filter.c:337-357) in float64"""
    n = np.arange(M)
    p = 2.0 * n / (M - 1) - 1.0
    return np.i0(np.pi * beta * np.sqrt(np.maximum(0.0, 1.0 - p * p))) / np.i0(np.pi * beta)


def bins_hz(N, Fc):
    k = np.arange(N)
    return np.where(k < N // 2, k, k - N) * Fc / N


def window_taps(R, M, beta):
    """window_filter (filter.c:365-413): ideal response R on N bins -> the M taps b, centred on M // 2 (the kernels use
    DFT_N(b zero padded))"""
    N = len(R)
    t = np.fft.ifft(R) * N
    n = np.arange(M)
    return t[(n - M // 2 + N) % N] * kaiser(M, beta) / N


def multiplex(n, Fc, left, right, pilot=0.1, pilot_hz=PILOT_HZ, deviation_hz=75000.0, phase=0.3):
    """the composite in rad/sample of 0.45 (L + R) + 0.45 (L - R) cos 2 theta + pilot cos theta at peak deviation"""
    theta = 2 * np.pi * pilot_hz * np.arange(n) / Fc + phase
    left = np.broadcast_to(np.asarray(left, np.float64), (n,))
    right = np.broadcast_to(np.asarray(right, np.float64), (n,))
    pil = np.broadcast_to(np.asarray(pilot, np.float64), (n,))
    m = 0.45 * (left + right) + 0.45 * (left - right) * np.cos(2 * theta) + pil * np.cos(theta)
    return 2 * np.pi * deviation_hz / Fc * m


def params(source=0, deviation_hz=75000.0, deemph_us=75.0, pilot_on_db=20.0, pilot_off_db=14.0, pilot_min_hz=2000.0,
           pilot_tol_hz=20.0, force_mono=0):
    return dict(source=source, deviation_hz=deviation_hz, deemph_us=deemph_us, pilot_on_db=pilot_on_db,
                pilot_off_db=pilot_off_db, pilot_min_hz=pilot_min_hz, pilot_tol_hz=pilot_tol_hz, force_mono=force_mono)


class WfmModel:
    def __init__(self, comp_rate, decimate, L, M, kaiser_beta=3.0, pilot_bw=1000.0):
        self.Fc, self.Da, self.L, self.M = float(comp_rate), decimate, L, M
        self.N, self.D = L + M - 1, (M - 1) // 2
        self.beta = f32(kaiser_beta)
        f = bins_hz(self.N, self.Fc)
        self.hp = window_taps(np.where(np.abs(f - PILOT_HZ) <= f32(pilot_bw) / 2, 1.0, 0.0), M, self.beta)

    def mono_taps(self, deemph_us):
        f = bins_hz(self.N, self.Fc)
        tau = f32(deemph_us) * 1e-6
        R = np.where(np.abs(f) <= AUDIO_HZ, 1.0 / (1.0 + 2j * np.pi * f * tau), 0.0)
        return window_taps(R, self.M, self.beta).real

    def decode(self, x, **kw):
        """x: the composite from stream index 0 (zeros before the slot's start).  -> (out [F L / Da][2], status dict of
        arrays [F]: pilot_hz, pilot_dev_hz, pilot_snr_db, stereo) for the F = len(x) // L completed frames"""
        p = params(**kw)
        x = np.asarray(x, np.float64)
        n, L, D, Fc = len(x), self.L, self.D, self.Fc
        F = n // L
        pil = np.convolve(x, self.hp)[:n]
        mag = np.abs(pil)
        u = np.where(mag > 0, pil / np.where(mag > 0, mag, 1.0), 0.0)
        xd = np.concatenate([np.zeros(D), x[:n - D]])
        d = 2 * xd * np.real(u * u)
        hm = self.mono_taps(p["deemph_us"])
        a = np.concatenate([np.zeros(D), np.convolve(x, hm)[:n - D]])
        s = np.convolve(d, hm)[:n]
        hz, dev, snr = np.zeros(F), np.zeros(F), np.zeros(F)
        k = np.arange(L)
        for f in range(F):
            seg = pil[f * L:(f + 1) * L]
            w = np.angle(np.sum(seg[1:] * np.conj(seg[:-1])))
            C = abs(np.mean(seg * np.exp(-1j * w * k))) ** 2
            T = np.mean(np.abs(seg) ** 2)
            hz[f] = w * Fc / (2 * np.pi)
            dev[f] = 2 * np.sqrt(C) * Fc / (2 * np.pi)
            with np.errstate(divide="ignore"):
                snr[f] = 10 * np.log10(C / (T - C)) if T - C > 0 else 100.0
        stereo = flags(hz, dev, snr, p)
        g = Fc / (2 * np.pi * 0.9 * f32(p["deviation_hz"]))
        j = np.arange(F * L // self.Da) * self.Da
        sg = stereo[j // L].astype(np.float64)
        out = np.stack([g * (a[j] + sg * s[j]), g * (a[j] - sg * s[j])], axis=1)
        return out, dict(pilot_hz=hz, pilot_dev_hz=dev, pilot_snr_db=snr, stereo=stereo)


def flags(hz, dev, snr, p, on=0):
    """the hysteresis over frames in order, from state `on`; force_mono pins sigma to 0"""
    out = np.zeros(len(hz), np.int32)
    for f in range(len(hz)):
        rest = dev[f] >= f32(p["pilot_min_hz"]) and abs(hz[f] - PILOT_HZ) <= f32(p["pilot_tol_hz"])
        on = int(rest and not snr[f] < f32(p["pilot_off_db"])) if on else int(rest and snr[f] >= f32(p["pilot_on_db"]))
        out[f] = 0 if p["force_mono"] else on
    return out


def tone_amp(y, rate, hz):
    """least-squares amplitude of a tone of hz in y"""
    t = np.arange(len(y)) / rate
    A = np.stack([np.cos(2 * np.pi * hz * t), np.sin(2 * np.pi * hz * t), np.ones_like(t)], axis=1)
    c = np.linalg.lstsq(A, y, rcond=None)[0]
    return float(np.hypot(c[0], c[1]))
