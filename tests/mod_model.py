"""CPU model of the modulator bank's contract (include/ka9q_hip.h, kq_mod_*), built from the oracle's pieces.

Two forms of the same contract:
  OracleStation  one station exactly as modulate.c's loop runs it: the oracle's REAL-in / COMPLEX-out filter
                 (kqo_create_filter_input / kqo_create_filter_output / kqo_window_filter) and the reference's own osc.c
                 (kq_oracle.ref_osc_lib()) where it is built, else the oracle's restatement (kqo_set_osc / kqo_step_osc).
  BankModel      many stations at once in float64 numpy (batched FFTs, oscillator in closed form): fast enough for a
                 thousand stations; tests/test_mod_model.py holds it to OracleStation.
FM (not in the reference) is float64 numpy on top of either.
"""
import ctypes as C

import numpy as np

import kq_oracle as ko

SHRT_MAX = 32767
MODES = {  # modulate.c:70-94 (type, low, high, carrier); FM: +-3000 Hz audio band
    "am": (0, -5000.0, 5000.0, 1.0),
    "usb": (0, 0.0, 3000.0, 0.0),
    "lsb": (0, -3000.0, 0.0, 0.0),
    "ame": (0, 0.0, 3000.0, 1.0),
    "fm": (1, -3000.0, 3000.0, 0.0),
}


def station(mode="am", frequency=48000.0, amplitude_dbfs=-20.0, sweep=0.0, deviation=3000.0, kaiser_beta=3.0, low=None,
            high=None, carrier=None):
    t, lo, hi, car = MODES[mode]
    return dict(mod_type=t, low=lo if low is None else low, high=hi if high is None else high,
                carrier=car if carrier is None else carrier, kaiser_beta=kaiser_beta, deviation=deviation,
                frequency=frequency, sweep=sweep, amplitude_dbfs=amplitude_dbfs)


def target_response(samprate, L, M, interp, low, high):
    """modulate.c:113-128 for any interp, in float as the reference evaluates it"""
    N = L + M - 1
    f32 = np.float32
    i = np.arange(N)
    f = f32(samprate) * ((i.astype(f32)) / f32(N))
    f = np.where(f > f32(samprate // 2), f - f32(samprate), f).astype(f32)
    resp = np.zeros(N, np.complex64)
    resp[(f >= f32(low)) & (f <= f32(high))] = f32(interp / N)
    return resp


def design_response(samprate, L, M, interp, low, high, beta):
    """target_response windowed by the oracle's window_filter (modulate.c:130)"""
    resp = target_response(samprate, L, M, interp, low, high)
    assert ko.lib().kqo_window_filter(L, M, resp.ctypes.data, beta) == 0
    return resp


def _as(ptr, n, dtype):
    nf = n * (2 if dtype == np.complex64 else 1)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (nf,)).view(dtype)


class _FilterIn(C.Structure):   # kqo_filter_in (oracle/kq_oracle.h)
    _fields_ = [("in_type", C.c_int), ("ilen", C.c_uint), ("impulse_length", C.c_uint), ("n", C.c_uint),
                ("fdomain", C.c_void_p), ("inbuf_c", C.c_void_p), ("inbuf_r", C.c_void_p), ("input_c", C.c_void_p),
                ("input_r", C.c_void_p), ("blocknum", C.c_uint), ("plan", C.c_void_p)]


class _FilterOut(C.Structure):  # kqo_filter_out
    _fields_ = [("master", C.c_void_p), ("out_type", C.c_int), ("response", C.c_void_p), ("f_fdomain", C.c_void_p),
                ("noise_gain", C.c_float), ("outbuf_c", C.c_void_p), ("outbuf_r", C.c_void_p), ("output_c", C.c_void_p),
                ("output_r", C.c_void_p), ("decimate", C.c_uint), ("olen", C.c_uint), ("n_dec", C.c_uint),
                ("blocknum", C.c_uint), ("plan", C.c_void_p)]


class RefOsc:
    """struct osc driven through set_osc / step_osc: the reference's osc.c where oracle/_ref is built, else the oracle's"""

    def __init__(self):
        self.R = ko.ref_osc_lib()
        if self.R is not None:
            self.o = ko.RefOsc()
        else:
            self.O = ko.lib()
            self.o = ko.Osc()

    def set(self, f, r):
        (self.R.set_osc if self.R is not None else self.O.kqo_set_osc)(C.byref(self.o), f, r)

    def steps(self, n):
        step = self.R.step_osc if self.R is not None else self.O.kqo_step_osc
        out = np.empty(n, np.complex128)
        for i in range(n):
            z = step(C.byref(self.o))
            out[i] = complex(z.re, z.im)
        return out


class OracleStation:
    """One station through modulate.c's loop (modulate.c:131-163) on the oracle's filter and osc.c"""

    def __init__(self, samprate, L, M, interp, st):
        self.Fs, self.L, self.M, self.I = samprate, L, M, interp
        self.N = L + M - 1
        O = ko.lib()
        self.O = O
        self.m = O.kqo_create_filter_input(L, M, ko.KQO_REAL)
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        self.resp_ptr = libc.malloc(8 * self.N)   # the filter owns (and frees) its response
        self.s = O.kqo_create_filter_output(self.m, self.resp_ptr, 1, ko.KQO_COMPLEX)
        self.mi = C.cast(self.m, C.POINTER(_FilterIn)).contents
        self.so = C.cast(self.s, C.POINTER(_FilterOut)).contents
        self.osc = RefOsc()
        self.theta = 0.0
        self.st = None
        self.set(st)

    def set(self, st):
        """kq_mod_set_station on a running station: new response from the next block, osc retuned phase-continuously"""
        old = self.st
        if old is None or (old["low"], old["high"], old["kaiser_beta"]) != (st["low"], st["high"], st["kaiser_beta"]):
            r = design_response(self.Fs, self.L, self.M, self.I, st["low"], st["high"], st["kaiser_beta"])
            C.memmove(self.so.response, r.ctypes.data, 8 * self.N)
        if st["mod_type"] == 1 and (old is None or old["mod_type"] != 1):
            self.theta = 0.0
        self.osc.set(st["frequency"] / self.Fs, st["sweep"] / (float(self.Fs) * self.Fs))   # modulate.c:104-108
        self.amp = 10.0 ** (st["amplitude_dbfs"] / 20.0)
        self.st = dict(st)

    def block(self, audio):
        """audio: L / I float32 samples (already scaled) -> complex64[L], as modulate.c computes it (complex float)"""
        L, I = self.L, self.I
        x = np.zeros(L, np.float32)
        x[::I] = audio
        _as(self.mi.input_r, L, np.float32)[:] = x
        self.O.kqo_execute_filter_input(self.m)
        self.O.kqo_execute_filter_output(self.s)
        y = _as(self.so.output_c, L, np.complex64).copy()
        if self.st["mod_type"] == 1:
            th = self.theta + 2 * np.pi * (self.st["deviation"] / self.Fs) * np.cumsum(y.real.astype(np.float64))
            self.theta = float(np.fmod(th[-1], 2 * np.pi))
            bb = np.exp(1j * th)
        else:
            bb = y.astype(np.complex128) + np.float32(self.st["carrier"])
        return (bb * (self.osc.steps(L) * self.amp)).astype(np.complex64)

    def close(self):
        if self.s:
            self.O.kqo_delete_filter_output(self.s)
            self.O.kqo_delete_filter_input(self.m)
            self.s = self.m = None

    def __del__(self):
        self.close()


class BankModel:
    """The whole contract in float64 numpy: stations by slot, the sum of their outputs per block"""

    def __init__(self, samprate, L, M, interp):
        self.Fs, self.L, self.M, self.I = samprate, L, M, interp
        self.N = L + M - 1
        self.Na, self.Hn, self.La = self.N // interp, (M - 1) // interp, L // interp
        self.st, self.hist, self.osc, self.theta = {}, {}, {}, {}
        self._resp = {}

    def response(self, st):
        key = (np.float32(st["low"]), np.float32(st["high"]), np.float32(st["kaiser_beta"]))
        if key not in self._resp:
            self._resp[key] = design_response(self.Fs, self.L, self.M, self.I, *key).astype(np.complex128)
        return self._resp[key]

    def set_station(self, slot, st):
        Fs = float(self.Fs)
        if slot not in self.st:
            self.hist[slot] = np.zeros(self.Hn, np.float64)
            self.osc[slot] = [0.0, 0.0, 0.0]
            self.theta[slot] = 0.0
        elif st["mod_type"] == 1 and self.st[slot]["mod_type"] != 1:
            self.theta[slot] = 0.0
        o = self.osc[slot]
        o[1], o[2] = st["frequency"] / Fs, st["sweep"] / (Fs * Fs)
        self.st[slot] = dict(st)

    def remove_station(self, slot):
        for d in (self.st, self.hist, self.osc, self.theta):
            d.pop(slot, None)

    def station_block(self, slot, window):
        """window: Na audio samples -> this station's complex128[L] for one block; advances its state"""
        st, L, M, N = self.st[slot], self.L, self.M, self.N
        x = np.zeros(N)
        x[::self.I] = window
        X = np.fft.fft(x)
        y = np.fft.ifft(self.response(st) * X)[M - 1:] * N
        n = np.arange(L, dtype=np.float64)
        p, f, r = self.osc[slot]
        if f != 0.0:   # osc.c:44
            ph = p + n * (f + 0.5 * r * (n - 1))
            np_ = p + L * (f + 0.5 * r * (L - 1))
            self.osc[slot] = [np_ - np.rint(np_), f + r * L, r]
        else:
            ph = np.full(L, p)
        if st["mod_type"] == 1:
            th = self.theta[slot] + (st["deviation"] / self.Fs) * np.cumsum(y.real)
            self.theta[slot] = th[-1] - np.rint(th[-1])
            bb = np.exp(2j * np.pi * th)
        else:
            bb = y + np.float32(st["carrier"])
        return bb * np.exp(2j * np.pi * ph) * 10.0 ** (st["amplitude_dbfs"] / 20.0)

    def process(self, pcm, nblocks, per_station=False):
        """pcm: rows by slot, float (already scaled); -> (complex128[nblocks * L] sum, {slot: complex128[...]} if asked)"""
        L, La, Hn = self.L, self.La, self.Hn
        total = np.zeros(nblocks * L, np.complex128)
        each = {}
        for slot in sorted(self.st):
            stream = np.concatenate([self.hist[slot], np.asarray(pcm[slot][:nblocks * La], np.float64)])
            out = np.concatenate([self.station_block(slot, stream[b * La:b * La + self.Na]) for b in range(nblocks)])
            self.hist[slot] = stream[len(stream) - Hn:] if Hn else np.zeros(0)
            total += out
            if per_station:
                each[slot] = out
        return total, each


def to_s16(x):
    """modulate.c:160-163 with saturation"""
    v = np.asarray(x, np.complex64)
    re = np.clip(v.real * np.float32(SHRT_MAX), -32768, 32767)
    im = np.clip(v.imag * np.float32(SHRT_MAX), -32768, 32767)
    return np.stack([np.trunc(re), np.trunc(im)], axis=-1).astype(np.int16)
