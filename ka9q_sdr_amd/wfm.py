"""Python mirror of the wideband FM stereo decoder bank (include/ka9q_hip.h: kq_wfm_*): broadcast FM composites (the
discriminator output of flat FM channels, rad/sample) to left / right audio, up to 4096 slots.  ctypes over
libka9q_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library

MAX_SLOTS = 4096
PILOT_HZ = 19000.0
STATUS_DTYPE = np.dtype([("pilot_hz", np.float32), ("pilot_dev_hz", np.float32), ("pilot_snr_db", np.float32),
                         ("stereo", np.int32)])


class WfmConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("comp_rate", C.c_int), ("decimate", C.c_uint), ("L", C.c_uint), ("M", C.c_uint),
                ("kaiser_beta", C.c_float), ("pilot_bw", C.c_float), ("max_slots", C.c_uint), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class WfmParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("deviation_hz", C.c_float), ("deemph_us", C.c_float), ("pilot_on_db", C.c_float),
                ("pilot_off_db", C.c_float), ("pilot_min_hz", C.c_float), ("pilot_tol_hz", C.c_float),
                ("force_mono", C.c_int)]


def wfm_params(source=0, deviation_hz=75000.0, deemph_us=75.0, pilot_on_db=20.0, pilot_off_db=14.0, pilot_min_hz=2000.0,
               pilot_tol_hz=20.0, force_mono=0):
    """kq_wfm_params with broadcast defaults: 75 kHz deviation, 75 us de-emphasis, stereo on at 20 dB pilot SNR, off below
    14 dB, with at least 2 kHz of pilot deviation within 20 Hz of 19 kHz"""
    return WfmParams(source, deviation_hz, deemph_us, pilot_on_db, pilot_off_db, pilot_min_hz, pilot_tol_hz, int(force_mono))


def _bind(L):
    if getattr(L, "_kq_wfm_bound", False):
        return L
    L.kq_wfm_create.restype = C.c_void_p
    L.kq_wfm_create.argtypes = [C.POINTER(WfmConfig)]
    L.kq_wfm_destroy.argtypes = [C.c_void_p]
    L.kq_wfm_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(WfmParams)]
    L.kq_wfm_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_wfm_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_size_t]
    L.kq_wfm_sync.argtypes = [C.c_void_p]
    L.kq_wfm_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_wfm_bound = True
    return L


class WfmBank(Handle):
    """Up to max_slots stereo decoders on one composite geometry (Fc = comp_rate, Da = decimate, frames of L, filters of M).
    For process_bank, create it on the receiver bank's stream: WfmBank.beside(bank, ...)."""
    _destroy = "kq_wfm_destroy"

    def __init__(self, comp_rate, decimate, L, M, max_slots, max_samples, kaiser_beta=3.0, pilot_bw=1000.0, device=0,
                 stream=None):
        self.lib = _bind(load_library())
        cfg = WfmConfig(device, comp_rate, decimate, L, M, kaiser_beta, pilot_bw, max_slots, max_samples, stream)
        self.h = self.lib.kq_wfm_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_wfm_create: " + _err(self.lib))
        self.comp_rate, self.decimate, self.L, self.M = comp_rate, decimate, L, M
        self.max_slots, self.max_samples, self.device, self.stream = max_slots, max_samples, device, stream
        self.out_rate = comp_rate / decimate
        self.n = 0   # composite samples taken so far

    @classmethod
    def beside(cls, bank, decimate, L, M, max_slots, kaiser_beta=3.0, pilot_bw=1000.0):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D)"""
        lib = _bind(load_library())
        rate = bank.samprate // bank.D
        return cls(rate, decimate, L, M, max_slots, bank.max_blocks * bank.olen, kaiser_beta, pilot_bw,
                   stream=lib.kq_bank_stream(bank.h))

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (a WfmParams, or wfm_params() keywords); it starts cold at the next call"""
        p = params if params is not None else wfm_params(**kw)
        self._chk(self.lib.kq_wfm_set(self.h, slot, C.byref(p)), "kq_wfm_set")

    def remove(self, slot):
        self._chk(self.lib.kq_wfm_remove(self.h, slot), "kq_wfm_remove")

    def frames(self, nsamples):
        """frames the next call of nsamples completes"""
        return (self.n + nsamples) // self.L - self.n // self.L

    def process(self, comp, nblocks=1):
        """comp: host float32 [rows][n] (row = source), n split into nblocks equal blocks.  Synchronous.  Returns
        (out float32 [max_slots][F L / Da][2] (L, R), status STATUS_DTYPE [max_slots][F]); rows of empty slots are 0."""
        comp = np.ascontiguousarray(comp, np.float32)
        if comp.ndim == 1:
            comp = comp[None, :]
        n = comp.shape[1]
        if n % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (n, nblocks))
        F = self.frames(n)
        lo = F * self.L // self.decimate
        out = np.zeros((self.max_slots, lo, 2), np.float32)
        st = np.zeros((self.max_slots, F), STATUS_DTYPE)
        got = self._chk(self.lib.kq_wfm_process(self.h, comp.ctypes.data, n, n // nblocks, n // nblocks, nblocks, 0,
                                                out.ctypes.data, 2 * lo, st.ctypes.data, F), "kq_wfm_process")
        assert got == F
        self.n += n
        return out, st

    def process_device(self, comp_ptr, src_stride, row_stride, block_len, nblocks, out_ptr=None, out_stride=0,
                       status_ptr=None, status_stride=0):
        """asynchronous on the handle's stream; every pointer is device memory.  Returns F."""
        F = self._chk(self.lib.kq_wfm_process(self.h, comp_ptr, src_stride, row_stride, block_len, nblocks, 1, out_ptr,
                                              out_stride, status_ptr, status_stride), "kq_wfm_process")
        self.n += block_len * nblocks
        return F

    def process_bank(self, bank, out=None, status=None):
        """Decode a receiver Bank's last call straight from its device audio plane (flat FM channels: the composite) on the
        bank's stream, with no host round trip and no host wait: kq_bank_join first orders the decode behind the bank's
        demodulators, wherever the bank ran them.  out / status: contiguous torch device tensors float32
        [max_slots][>= F L / Da][2] and int32 [max_slots][>= F][4] to write, or None for new zeroed ones.  Returns
        (F, out[:, :F L / Da], status[:, :F]); status_array() views a status tensor as STATUS_DTYPE.  The decode waits for
        what torch's current stream has queued, and that stream waits for the decode, so the tensors are used there as
        any others."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs a WfmBank on the bank's stream (WfmBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        F = self.frames(nb * olen)
        lo = F * self.L // self.decimate
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((self.max_slots, max(lo, 1), 2), dtype=torch.float32, device=dev)
        if status is None:
            status = torch.zeros((self.max_slots, max(F, 1), 4), dtype=torch.int32, device=dev)
        if not (out.is_contiguous() and status.is_contiguous()) or out.shape[1] < lo or status.shape[1] < F:
            raise ValueError("out / status must be contiguous and hold %d outputs / %d frames per slot" % (lo, F))
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the decoder writes them
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        got = self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, out.data_ptr(),
                                  2 * out.shape[1], status.data_ptr(), status.shape[1])
        assert got == F
        # torch's stream waits for the decode, so a later use or reuse of the buffers there comes after it.  (No
        # record_stream on the bank's stream: the allocator would record on it when the tensors are freed, perhaps after
        # the bank that owns the stream has destroyed it.)
        cur.wait_stream(ext)
        return F, out[:, :lo], status[:, :F]

    def sync(self):
        self._chk(self.lib.kq_wfm_sync(self.h), "kq_wfm_sync")

    def reset(self):
        self._chk(self.lib.kq_wfm_reset(self.h), "kq_wfm_reset")
        self.n = 0


def status_array(st):
    """a status tensor / int32 array [..][4] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


__all__ = ["WfmBank", "WfmConfig", "WfmParams", "wfm_params", "status_array", "STATUS_DTYPE", "MAX_SLOTS"]
