"""Python mirror of the raw A/D conditioning stage (include/ka9q_hip.h: kq_fe_*).

Mirrors what hackrf.c:122-196 (rx_callback) and funcube.c:287-390 do to every sample off the A/D before the cascade:
integer to float, DC removal, I/Q gain balance, I/Q phase correction, and the running estimates behind them.  ctypes over
libka9q_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library
from .decimate import Decimator, _bind as _bind_decim

KQ_FE_S8 = 0
KQ_FE_S16 = 1


class FeConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("format", C.c_int), ("block", C.c_uint), ("adc_samprate", C.c_double),
                ("dc_alpha", C.c_double), ("power_alpha", C.c_double), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class FeStatus(C.Structure):
    _fields_ = [("samples", C.c_ulonglong), ("blocks", C.c_ulonglong), ("clips", C.c_ulonglong),
                ("DC_i", C.c_float), ("DC_q", C.c_float), ("imbalance", C.c_float), ("sinphi", C.c_float),
                ("in_power", C.c_float), ("gain_i", C.c_float), ("gain_q", C.c_float), ("secphi", C.c_float),
                ("tanphi", C.c_float), ("reserved_", C.c_float)]


# one kq_fe_status record as a numpy row (block_status of a call is an array of these)
FE_STATUS_DTYPE = np.dtype([("samples", "<u8"), ("blocks", "<u8"), ("clips", "<u8"), ("DC_i", "<f4"), ("DC_q", "<f4"),
                            ("imbalance", "<f4"), ("sinphi", "<f4"), ("in_power", "<f4"), ("gain_i", "<f4"),
                            ("gain_q", "<f4"), ("secphi", "<f4"), ("tanphi", "<f4"), ("reserved_", "<f4")])
assert FE_STATUS_DTYPE.itemsize == C.sizeof(FeStatus) == 64


def _bind(L):
    if getattr(L, "_kq_fe_bound", False):
        return L
    L.kq_fe_create.restype = C.c_void_p
    L.kq_fe_create.argtypes = [C.POINTER(FeConfig)]
    for name in ("kq_fe_destroy", "kq_fe_reset", "kq_fe_sync"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.kq_fe_stream.restype = C.c_void_p
    L.kq_fe_stream.argtypes = [C.c_void_p]
    L.kq_fe_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kq_fe_process_decim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    L.kq_fe_get_status.argtypes = [C.c_void_p, C.POINTER(FeStatus)]
    L._kq_fe_bound = True
    return L


class FrontEnd(Handle):
    """Conditioning of raw int8 / int16 I,Q samples with carried estimates, updated every `block` samples of the stream.

    dc_alpha defaults to the reference's value for the format (hackrf.c:74 1e-7, funcube.c:65 1e-6), power_alpha to its
    1.0.  decimator=dict(log_decimate=..., ...) also creates a Decimator on this handle's stream (self.decimator), which
    process_decim then uses."""
    _destroy = "kq_fe_destroy"

    def __init__(self, fmt, block, adc_samprate, dc_alpha=None, power_alpha=1.0, max_samples=1 << 20, device=0,
                 stream=None, decimator=None):
        self.lib = self.L = _bind_decim(_bind(load_library()))
        if dc_alpha is None:
            dc_alpha = 1e-6 if fmt == KQ_FE_S16 else 1e-7
        cfg = FeConfig(device, fmt, block, adc_samprate, dc_alpha, power_alpha, max_samples, stream)
        self.decimator = None
        self.h = self.L.kq_fe_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_fe_create: " + _err(self.L))
        self.format, self.block, self.max_samples = fmt, block, max_samples
        self.stream = self.L.kq_fe_stream(self.h)
        if decimator is not None:
            kw = dict(decimator)
            kw.setdefault("max_out", max(1, max_samples >> kw["log_decimate"]))
            self.decimator = Decimator(device=device, stream=self.stream, **kw)

    def close(self):
        if getattr(self, "decimator", None) is not None:
            self.decimator.close()
            self.decimator = None
        super().close()

    def _raw(self, raw):
        raw = np.ascontiguousarray(raw, np.int16 if self.format == KQ_FE_S16 else np.int8)
        if raw.ndim != 2 or raw.shape[1] != 2:
            raise ValueError("raw samples are an array of I,Q pairs, shape (n, 2)")
        return raw

    def process(self, raw, want_cf32=True, want_s16=False):
        """raw: int8 / int16 [n, 2] on the host -> (complex64[n] | None, int16[n, 2] | None, block status records)"""
        raw = self._raw(raw)
        n = len(raw)
        out = np.empty(n, np.complex64) if want_cf32 else None
        s16 = np.empty((n, 2), np.int16) if want_s16 else None
        st = np.zeros(n // self.block + 2, FE_STATUS_DTYPE)
        rc = self._chk(self.L.kq_fe_process(self.h, raw.ctypes.data, 0, n, out.ctypes.data if want_cf32 else None,
                                            s16.ctypes.data if want_s16 else None, st.ctypes.data), "kq_fe_process")
        return out, s16, st[:rc]

    def process_device(self, raw_ptr, n, out_ptr=None, s16_ptr=None, status_ptr=None):
        """Asynchronous, device pointers on the handle's stream; returns the number of blocks completed in the call."""
        return self._chk(self.L.kq_fe_process(self.h, raw_ptr, 1, n, out_ptr, s16_ptr, status_ptr), "kq_fe_process")

    def process_decim(self, raw, decimator=None, want_s16=True):
        """raw: int8 / int16 [n_out << log_decimate, 2] on the host, conditioned and decimated in one pass ->
        (complex64[n_out], int16[n_out, 2] | None, energy, block status records)"""
        dec = decimator if decimator is not None else self.decimator
        raw = self._raw(raw)
        n_out = len(raw) >> dec.log_decimate
        if n_out << dec.log_decimate != len(raw):
            raise ValueError("input length must be a multiple of the decimation ratio")
        out = np.empty(n_out, np.complex64)
        s16 = np.empty((n_out, 2), np.int16) if want_s16 else None
        energy = C.c_float(0)
        st = np.zeros(len(raw) // self.block + 2, FE_STATUS_DTYPE)
        rc = self._chk(self.L.kq_fe_process_decim(self.h, dec.h, raw.ctypes.data, 0, n_out, out.ctypes.data,
                                                  s16.ctypes.data if want_s16 else None, C.addressof(energy),
                                                  st.ctypes.data), "kq_fe_process_decim")
        return out, s16, energy.value, st[:rc]

    def process_decim_device(self, raw_ptr, n_out, out_ptr, s16_ptr=None, energy_ptr=None, status_ptr=None,
                             decimator=None):
        """Asynchronous, device pointers on the handle's stream; returns the number of blocks completed in the call."""
        dec = decimator if decimator is not None else self.decimator
        return self._chk(self.L.kq_fe_process_decim(self.h, dec.h, raw_ptr, 1, n_out, out_ptr, s16_ptr, energy_ptr,
                                                    status_ptr), "kq_fe_process_decim")

    def status(self):
        """The state after the last completed block (waits for the stream), as one FE_STATUS_DTYPE record."""
        st = FeStatus()
        self._chk(self.L.kq_fe_get_status(self.h, C.byref(st)), "kq_fe_get_status")
        return np.frombuffer(bytes(st), FE_STATUS_DTYPE)[0]

    def reset(self):
        self._chk(self.L.kq_fe_reset(self.h), "kq_fe_reset")
        if self.decimator is not None:
            self.decimator.reset()

    def sync(self):
        self._chk(self.L.kq_fe_sync(self.h), "kq_fe_sync")
