"""Python mirror of the spectrum bank (include/ka9q_hip.h: kq_spec_*): averaged power spectra of the wideband I/Q stream,
many analyzers (overviews, zooms, Doppler-following views) over one stream.  ctypes over libka9q_hip.so; there is no CPU
path.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from .bank import KQ_IQ_CF32, KQ_IQ_S16, KQ_IQ_S8, Handle, KqError, _err, load_library

MAX_SPECS, MAX_DECIMATE, MIN_FFT, MAX_FFT = 4096, 256, 16, 16384


class SpecConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_int), ("gain_factor", C.c_float), ("max_specs", C.c_uint),
                ("max_samples", C.c_size_t), ("max_rows", C.c_uint), ("stream", C.c_void_p)]


class SpecParams(C.Structure):
    _fields_ = [("center", C.c_double), ("sweep", C.c_double), ("decimate", C.c_uint), ("fft_size", C.c_uint),
                ("bins", C.c_uint), ("hop", C.c_uint), ("average", C.c_uint), ("kaiser_beta", C.c_float)]


class SpecRow(C.Structure):
    _fields_ = [("start_sample", C.c_uint64), ("frames", C.c_uint32), ("generation", C.c_uint32)]


class SpecInfo(C.Structure):
    _fields_ = [("bin_bw", C.c_double), ("first_bin_hz", C.c_double), ("enbw_bins", C.c_double),
                ("delay_samples", C.c_double), ("rows_ready", C.c_uint64), ("rows_dropped", C.c_uint64),
                ("frames_pending", C.c_uint32), ("generation", C.c_uint32)]


def spec_params(fft_size, bins=None, decimate=1, center=0.0, sweep=0.0, hop=None, average=1, kaiser_beta=3.0):
    """kq_spec_params with defaults: every bin the size allows (Nf at Dz = 1, 3 Nf / 4 when zoomed), 50 % overlap"""
    if bins is None:
        bins = fft_size if decimate == 1 else (3 * fft_size // 4) & ~1
    return SpecParams(center, sweep, decimate, fft_size, bins, fft_size // 2 if hop is None else hop, average, kaiser_beta)


def served_size(n):
    """an FFT size the bank serves: even, 2^a 3^b 5^c 7^d, 16 .. 16384"""
    if n < MIN_FFT or n > MAX_FFT or n % 2:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def plan(samprate, bin_bw, bins):
    """(decimate, fft_size) with decimate * fft_size == samprate / bin_bw exactly, fft_size served and at or above the bins
    limit (bins <= fft_size at decimate 1, bins <= 3 fft_size / 4 above), decimate <= 256: the smallest such fft_size.
    ValueError with the reason when there is none."""
    prod = Fraction(samprate) / Fraction(bin_bw)
    if prod.denominator != 1:
        raise ValueError("samprate / bin_bw = %s is not an integer: no decimate * fft_size gives %g Hz bins" % (prod, bin_bw))
    P = prod.numerator
    if bins < 2 or bins % 2:
        raise ValueError("bins %d must be even and positive" % bins)
    for nf in range(MIN_FFT, MAX_FFT + 1, 2):
        if P % nf or not served_size(nf):
            continue
        dz = P // nf
        if dz > MAX_DECIMATE:
            continue
        if (dz == 1 and bins <= nf) or (dz > 1 and 4 * bins <= 3 * nf):
            return dz, nf
    raise ValueError("no decimate <= %d and served fft_size with decimate * fft_size = %d (samprate %g / bin_bw %g) keeps %d "
                     "bins" % (MAX_DECIMATE, P, samprate, bin_bw, bins))


def _bind(L):
    if getattr(L, "_kq_spec_bound", False):
        return L
    L.kq_spec_create.restype = C.c_void_p
    L.kq_spec_create.argtypes = [C.POINTER(SpecConfig)]
    L.kq_spec_destroy.argtypes = [C.c_void_p]
    L.kq_spec_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(SpecParams)]
    L.kq_spec_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_spec_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int]
    L.kq_spec_pull.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p]
    L.kq_spec_get_info.argtypes = [C.c_void_p, C.c_uint, C.POINTER(SpecInfo)]
    L.kq_spec_sync.argtypes = [C.c_void_p]
    L.kq_spec_reset.argtypes = [C.c_void_p]
    L._kq_spec_bound = True
    return L


def _iq_format(dtype, shape):
    """(format, nsamples) of an I/Q array: complex64 [n], or int16 / int8 [n, 2] (or flat, interleaved)"""
    if dtype == np.complex64:
        return KQ_IQ_CF32, int(np.prod(shape))
    if dtype == np.int16:
        return KQ_IQ_S16, int(np.prod(shape)) // 2
    if dtype == np.int8:
        return KQ_IQ_S8, int(np.prod(shape)) // 2
    raise TypeError("I/Q must be complex64, int16 or int8 (got %s)" % dtype)


class SpecBank(Handle):
    """Up to max_specs analyzers over one I/Q stream of samprate samples per second."""
    _destroy = "kq_spec_destroy"

    def __init__(self, samprate, max_specs, max_samples, max_rows=64, gain_factor=1.0, device=0, stream=None):
        self.lib = _bind(load_library())
        cfg = SpecConfig(device, samprate, gain_factor, max_specs, max_samples, max_rows, stream)
        self.h = self.lib.kq_spec_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_spec_create: " + _err(self.lib))
        self.samprate, self.max_specs, self.max_samples, self.max_rows = samprate, max_specs, max_samples, max_rows
        self._bins = {}

    def set(self, slot, params=None, **kw):
        """add or replace the analyzer in `slot`: a SpecParams, or spec_params() keywords"""
        p = params if params is not None else spec_params(**kw)
        self._chk(self.lib.kq_spec_set(self.h, slot, C.byref(p)), "kq_spec_set")
        self._bins[slot] = p.bins

    def remove(self, slot):
        self._chk(self.lib.kq_spec_remove(self.h, slot), "kq_spec_remove")
        self._bins.pop(slot, None)

    def process(self, iq):
        """iq: a host numpy array (synchronous) or a torch device tensor (asynchronous on the bank's stream): complex64 [n],
        or int16 / int8 [n, 2]"""
        if hasattr(iq, "data_ptr"):
            import torch
            if not iq.is_cuda:
                iq = iq.numpy()
            else:
                if not iq.is_contiguous():
                    raise ValueError("device I/Q must be contiguous")
                dt = {torch.complex64: np.complex64, torch.int16: np.int16, torch.int8: np.int8}.get(iq.dtype)
                if dt is None:
                    raise TypeError("I/Q must be complex64, int16 or int8 (got %s)" % iq.dtype)
                fmt, n = _iq_format(dt, tuple(iq.shape))
                self._chk(self.lib.kq_spec_process(self.h, iq.data_ptr(), fmt, n, 1), "kq_spec_process")
                return
        iq = np.ascontiguousarray(iq)
        fmt, n = _iq_format(iq.dtype, iq.shape)
        self._chk(self.lib.kq_spec_process(self.h, iq.ctypes.data if n else None, fmt, n, 0), "kq_spec_process")

    def process_device(self, ptr, fmt, nsamples):
        """asynchronous, a raw device pointer on the bank's stream"""
        self._chk(self.lib.kq_spec_process(self.h, ptr, fmt, nsamples, 1), "kq_spec_process")

    def pull(self, slot, max_rows=None):
        """(rows float32 [n, B], start_sample uint64 [n], generation uint32 [n]) of the slot's oldest rows"""
        B = self._bins[slot]
        cap = self.max_rows if max_rows is None else max_rows
        rows = np.empty((cap, B), np.float32)
        meta = (SpecRow * max(cap, 1))()
        n = self._chk(self.lib.kq_spec_pull(self.h, slot, rows.ctypes.data, cap, meta), "kq_spec_pull")
        start = np.array([meta[i].start_sample for i in range(n)], np.uint64)
        gen = np.array([meta[i].generation for i in range(n)], np.uint32)
        return rows[:n], start, gen

    def info(self, slot):
        i = SpecInfo()
        self._chk(self.lib.kq_spec_get_info(self.h, slot, C.byref(i)), "kq_spec_get_info")
        return {f: getattr(i, f) for f, _ in SpecInfo._fields_}

    def sync(self):
        self._chk(self.lib.kq_spec_sync(self.h), "kq_spec_sync")

    def reset(self):
        self._chk(self.lib.kq_spec_reset(self.h), "kq_spec_reset")


__all__ = ["SpecBank", "SpecConfig", "SpecParams", "SpecRow", "SpecInfo", "spec_params", "plan", "served_size",
           "KQ_IQ_CF32", "KQ_IQ_S16", "KQ_IQ_S8"]
