"""Python mirror of the rational resampler bank (include/ka9q_hip.h: kq_rsmp_*): up to 65536 slots, each one row of PCM
(mono or stereo) from Fi = in_rate_num / in_rate_den Hz to Fo = out_rate Hz through a polyphase Kaiser-windowed sinc.
ctypes over libka9q_hip.so; there is no CPU path.
"""
import ctypes as C
import math

import numpy as np

from .bank import Handle, KqError, _err, load_library
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 65536
TILE_MAX, SPAN = 1024, 4096     # k_rsmp: outputs per workgroup at most, input samples per side it stages


class RsmpConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("in_rate_num", C.c_int), ("in_rate_den", C.c_int), ("out_rate", C.c_int),
                ("taps", C.c_uint), ("cutoff_hz", C.c_float), ("kaiser_beta", C.c_float), ("max_slots", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class RsmpParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("channels", C.c_int)]


class RsmpInfo(C.Structure):
    _fields_ = [("P", C.c_uint32), ("Q", C.c_uint32), ("taps", C.c_uint32), ("delay_in_samples", C.c_double),
                ("next_in", C.c_uint64), ("next_out", C.c_uint64)]


def rsmp_params(source=0, channels=1):
    """kq_rsmp_params: a mono slot on row 0"""
    return RsmpParams(source, channels)


def _bind(L):
    if getattr(L, "_kq_rsmp_bound", False):
        return L
    L.kq_rsmp_create.restype = C.c_void_p
    L.kq_rsmp_create.argtypes = [C.POINTER(RsmpConfig)]
    L.kq_rsmp_destroy.argtypes = [C.c_void_p]
    L.kq_rsmp_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(RsmpParams)]
    L.kq_rsmp_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_rsmp_max_out.restype = C.c_size_t
    L.kq_rsmp_max_out.argtypes = [C.c_void_p, C.c_size_t]
    L.kq_rsmp_get_info.argtypes = [C.c_void_p, C.POINTER(RsmpInfo)]
    L.kq_rsmp_get_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_rsmp_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.kq_rsmp_sync.argtypes = [C.c_void_p]
    L.kq_rsmp_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_rsmp_bound = True
    return L


class RsmpBank(Handle):
    """Up to max_slots resamplers on one pair of rates and one filter (taps per phase, cutoff_hz, kaiser_beta).  To run
    behind a receiver Bank on its device audio plane, create it on the bank's stream: RsmpBank.beside(bank, ...)."""
    _destroy = "kq_rsmp_destroy"

    def __init__(self, in_rate_num, in_rate_den, out_rate, taps, cutoff_hz, kaiser_beta, max_slots, max_samples, stream=None,
                 device=0):
        self.lib = _bind(load_library())
        cfg = RsmpConfig(device, in_rate_num, in_rate_den, out_rate, taps, cutoff_hz, kaiser_beta, max_slots, max_samples,
                         stream)
        self.h = self.lib.kq_rsmp_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_rsmp_create: " + _err(self.lib))
        self.max_slots, self.max_samples, self.device, self.stream = max_slots, max_samples, device, stream
        i = self.info()
        self.P, self.Q, self.T = i.P, i.Q, i.taps
        self.channels = {}   # slot -> 1 or 2

    @classmethod
    def beside(cls, bank, out_rate, taps, max_slots, cutoff_hz=None, kaiser_beta=3.0):
        """a resampler on a receiver Bank's stream, sized for its calls, from its output rate samprate / D; cutoff_hz
        defaults to clean_cutoff()"""
        lib = _bind(load_library())
        if cutoff_hz is None:
            cutoff_hz = cls.clean_cutoff(bank.samprate / bank.D, out_rate, taps, kaiser_beta)
        return cls(bank.samprate, bank.D, out_rate, taps, cutoff_hz, kaiser_beta, max_slots, bank.max_blocks * bank.olen,
                   stream=lib.kq_bank_stream(bank.h))

    @staticmethod
    def transition_hz(fi, taps, beta):
        """the width of the transition band: the Kaiser window's main lobe, about 2 fi sqrt(1 + beta^2) / taps"""
        return 2.0 * fi * math.sqrt(1.0 + beta * beta) / taps

    @staticmethod
    def clean_cutoff(fi, fo, taps, beta):
        """the cutoff_hz of a design with no aliasing: min(fi, fo) / 2 minus half of the transition band"""
        return 0.5 * min(fi, fo) - 0.5 * RsmpBank.transition_hz(fi, taps, beta)

    @property
    def tile(self):
        """outputs per workgroup of k_rsmp (a seam for the tests)"""
        return min(TILE_MAX, 1 + (SPAN - self.T - 1) * self.P // self.Q)

    def set(self, slot, params=None, **kw):
        """put a resampler in `slot` (an RsmpParams, or rsmp_params() keywords): zero history from the next call"""
        p = params if params is not None else rsmp_params(**kw)
        self._chk(self.lib.kq_rsmp_set(self.h, slot, C.byref(p)), "kq_rsmp_set")
        self.channels[slot] = p.channels

    def remove(self, slot):
        self._chk(self.lib.kq_rsmp_remove(self.h, slot), "kq_rsmp_remove")
        self.channels.pop(slot, None)

    def info(self):
        """kq_rsmp_info: P, Q, taps, delay_in_samples, next_in, next_out"""
        i = RsmpInfo()
        self._chk(self.lib.kq_rsmp_get_info(self.h, C.byref(i)), "kq_rsmp_get_info")
        return i

    def taps(self):
        """g[phi][k] as used, float32 [P][T]"""
        g = np.zeros((self.P, self.T), np.float32)
        assert self._chk(self.lib.kq_rsmp_get_taps(self.h, g.ctypes.data, g.size), "kq_rsmp_get_taps") == g.size
        return g

    def max_out(self, n):
        """ceil(n P / Q): the outputs of a call of n samples never exceed it"""
        return int(self.lib.kq_rsmp_max_out(self.h, n))

    def process(self, x, block_len=None, nblocks=1, row_stride=None, want_out=True, want_pcm=True, fill=0):
        """x: host array [rows][W] (row = source), float32 or int16 words in network byte order (dtype ">i2"); block k of
        a row starts at k row_stride (default W // nblocks) and holds block_len samples (default that too), interleaved
        pairs for a stereo slot.  Synchronous.  Returns (J, out float32 [max_slots][c J], pcm int16 [max_slots][c J] in
        host byte order), c = 2 where a stereo slot is set, else 1; rows of empty slots and what a mono slot leaves of a
        stereo row keep `fill`; an output not wanted is None."""
        x = np.asarray(x)
        if x.dtype.kind == "i" and x.dtype.itemsize == 2:
            fmt = KQ_PCM_S16BE
        else:
            fmt, x = KQ_PCM_F32, np.asarray(x, np.float32)
        x = np.ascontiguousarray(x)
        if x.ndim == 1:
            x = x[None, :]
        W = x.shape[1]
        if row_stride is None:
            row_stride = W // nblocks
        if block_len is None:
            block_len = row_stride
        c = 2 if 2 in self.channels.values() else 1
        i = self.info()
        n1 = i.next_in + block_len * nblocks
        J = -(-n1 * self.P // self.Q) - i.next_out
        w = max(c * J, 1)
        out = np.full((self.max_slots, w), fill, np.float32) if want_out else None
        pcm = np.full((self.max_slots, w), fill, ">i2") if want_pcm else None
        got = self._chk(self.lib.kq_rsmp_process(self.h, x.ctypes.data, fmt, W, row_stride, block_len, nblocks, 0,
                                                 out.ctypes.data if want_out else None, w,
                                                 pcm.ctypes.data if want_pcm else None, w), "kq_rsmp_process")
        assert got == J
        return J, (out[:, :c * J] if want_out else None), (pcm[:, :c * J].astype(np.int16) if want_pcm else None)

    def process_device(self, src_ptr, fmt, src_stride, row_stride, block_len, nblocks, out_ptr=None, out_stride=0,
                       pcm_ptr=None, pcm_stride=0):
        """asynchronous on the handle's stream; every pointer is device memory.  Returns J."""
        return self._chk(self.lib.kq_rsmp_process(self.h, src_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, out_ptr,
                                                  out_stride, pcm_ptr, pcm_stride), "kq_rsmp_process")

    def process_bank(self, bank, out, pcm=None):
        """Resample a receiver Bank's last call straight from its device audio plane (slot source = channel index) on the
        bank's stream, with no host round trip and no host wait: kq_bank_join first orders it behind the bank's
        demodulators.  out / pcm: contiguous torch device tensors float32 / int16 [max_slots][>= c J] to write (pcm in
        network byte order; either may be None).  Returns J.  The work waits for what torch's current stream has queued,
        and that stream waits for the work."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs an RsmpBank on the bank's stream (RsmpBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        dev = torch.device("cuda", self.device)
        for t in (out, pcm):
            if t is not None and not (t.is_contiguous() and t.shape[0] >= self.max_slots):
                raise ValueError("out / pcm must be contiguous [max_slots][>= c J]")
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the resampler writes them
        bank.join()            # the demodulators that write the plane, before the resampler reads it
        J = self.process_device(bank.audio_device_ptr(), KQ_PCM_F32, bank.max_blocks * 2 * olen, 2 * olen, olen, nb,
                                out.data_ptr() if out is not None else None, out.shape[1] if out is not None else 0,
                                pcm.data_ptr() if pcm is not None else None, pcm.shape[1] if pcm is not None else 0)
        cur.wait_stream(ext)
        return J

    def sync(self):
        self._chk(self.lib.kq_rsmp_sync(self.h), "kq_rsmp_sync")

    def reset(self):
        self._chk(self.lib.kq_rsmp_reset(self.h), "kq_rsmp_reset")


__all__ = ["RsmpBank", "RsmpConfig", "RsmpParams", "RsmpInfo", "rsmp_params", "MAX_SLOTS"]
