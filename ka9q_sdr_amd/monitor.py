"""Python mirror of the monitor mixer bank (include/ka9q_hip.h: kq_mon_*): up to 65536 sessions, each one row of PCM with
a gain, a stereo position and a mute switch, summed into up to 256 stereo buses.  ctypes over libka9q_hip.so; there is no
CPU path.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library

MAX_SESSIONS = 65536
MAX_BUSES = 256
KQ_MON_F32 = 0
KQ_MON_S16BE = 1
STATUS_DTYPE = np.dtype([("peak_left", np.float32), ("peak_right", np.float32), ("clipped", np.int32),
                         ("sessions", np.int32), ("active", np.int32)])


class MonConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_int), ("max_sessions", C.c_uint), ("max_buses", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class MonParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("bus", C.c_uint), ("channels", C.c_int), ("gain", C.c_float), ("pan", C.c_float),
                ("muted", C.c_int)]


def mon_params(source=0, bus=0, channels=1, gain=1.0, pan=0.0, muted=0):
    """kq_mon_params: a mono session at unit gain in the centre of bus 0"""
    return MonParams(source, bus, channels, gain, pan, int(muted))


def _bind(L):
    if getattr(L, "_kq_mon_bound", False):
        return L
    L.kq_mon_create.restype = C.c_void_p
    L.kq_mon_create.argtypes = [C.POINTER(MonConfig)]
    L.kq_mon_destroy.argtypes = [C.c_void_p]
    L.kq_mon_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(MonParams)]
    L.kq_mon_adjust.argtypes = [C.c_void_p, C.c_uint, C.c_float, C.c_float, C.c_int]
    L.kq_mon_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_mon_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.kq_mon_sync.argtypes = [C.c_void_p]
    L.kq_mon_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_mon_bound = True
    return L


class MonBank(Handle):
    """Up to max_sessions sessions mixed into max_buses stereo buses at one sample rate.  For process_bank, create it on
    the receiver bank's stream: MonBank.beside(bank, ...)."""
    _destroy = "kq_mon_destroy"

    def __init__(self, samprate, max_sessions, max_buses, max_samples, device=0, stream=None):
        self.lib = _bind(load_library())
        cfg = MonConfig(device, samprate, max_sessions, max_buses, max_samples, stream)
        self.h = self.lib.kq_mon_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_mon_create: " + _err(self.lib))
        self.samprate, self.max_sessions, self.max_buses, self.max_samples = samprate, max_sessions, max_buses, max_samples
        self.device, self.stream = device, stream
        self.H = int(np.floor(0.001 * samprate + 0.5))   # frames of history, the longest delay
        self.n = 0   # frames taken so far

    @classmethod
    def beside(cls, bank, max_sessions, max_buses=1):
        """a mixer on a receiver Bank's stream, sized for its calls, at its output rate (samprate / D)"""
        lib = _bind(load_library())
        return cls(bank.samprate // bank.D, max_sessions, max_buses, bank.max_blocks * bank.olen,
                   stream=lib.kq_bank_stream(bank.h))

    def set(self, slot, params=None, **kw):
        """put a session in `slot` (a MonParams, or mon_params() keywords): a cold start at the next call"""
        p = params if params is not None else mon_params(**kw)
        self._chk(self.lib.kq_mon_set(self.h, slot, C.byref(p)), "kq_mon_set")

    def adjust(self, slot, gain, pan, muted=0):
        """new gain, position and mute switch from the next call; the session's history is kept"""
        self._chk(self.lib.kq_mon_adjust(self.h, slot, gain, pan, int(muted)), "kq_mon_adjust")

    def remove(self, slot):
        self._chk(self.lib.kq_mon_remove(self.h, slot), "kq_mon_remove")

    def process(self, audio, block_len, nblocks=1, row_stride=None):
        """audio: host array [rows][W] (row = source), float32 or int16 words in network byte order; block k of a row
        starts at k row_stride (default W // nblocks) and holds block_len frames, interleaved pairs for a stereo session.
        Synchronous.  Returns (out float32 [max_buses][T][2], pcm int16 [max_buses][T][2] in host byte order, status
        STATUS_DTYPE [max_buses])."""
        audio = np.asarray(audio)
        if audio.dtype.kind == "i" and audio.dtype.itemsize == 2:
            fmt = KQ_MON_S16BE
        else:
            fmt, audio = KQ_MON_F32, np.asarray(audio, np.float32)
        audio = np.ascontiguousarray(audio)
        if audio.ndim == 1:
            audio = audio[None, :]
        W = audio.shape[1]
        if row_stride is None:
            row_stride = W // nblocks
        T = block_len * nblocks
        out = np.zeros((self.max_buses, T, 2), np.float32)
        pcm = np.zeros((self.max_buses, T, 2), ">i2")
        st = np.zeros(self.max_buses, STATUS_DTYPE)
        got = self._chk(self.lib.kq_mon_process(self.h, audio.ctypes.data, fmt, W, row_stride, block_len, nblocks, 0,
                                                out.ctypes.data, 2 * T, pcm.ctypes.data, 2 * T, st.ctypes.data),
                        "kq_mon_process")
        assert got == T
        self.n += T
        return out, pcm.astype(np.int16), st

    def process_device(self, audio_ptr, fmt, src_stride, row_stride, block_len, nblocks, out_ptr=None, out_stride=0,
                       pcm_ptr=None, pcm_stride=0, status_ptr=None):
        """asynchronous on the handle's stream; every pointer is device memory.  Returns T."""
        T = self._chk(self.lib.kq_mon_process(self.h, audio_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, out_ptr,
                                              out_stride, pcm_ptr, pcm_stride, status_ptr), "kq_mon_process")
        self.n += T
        return T

    def process_bank(self, bank, out=None, pcm=None, status=None):
        """Mix a receiver Bank's last call straight from its device audio plane (session source = channel index) on the
        bank's stream, with no host round trip and no host wait: kq_bank_join first orders the mix behind the bank's
        demodulators, wherever the bank ran them.  out / pcm / status: contiguous torch device tensors float32
        [max_buses][>= T][2], int16 [max_buses][>= T][2] (network byte order) and int32 [max_buses][5] to write, or None
        for new zeroed ones.  Returns (T, out[:, :T], pcm[:, :T], status); status_array() views a status tensor as
        STATUS_DTYPE.  The mix waits for what torch's current stream has queued, and that stream waits for the mix, so
        the tensors are used there as any others."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs a MonBank on the bank's stream (MonBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        T = nb * olen
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((self.max_buses, max(T, 1), 2), dtype=torch.float32, device=dev)
        if pcm is None:
            pcm = torch.zeros((self.max_buses, max(T, 1), 2), dtype=torch.int16, device=dev)
        if status is None:
            status = torch.zeros((self.max_buses, 5), dtype=torch.int32, device=dev)
        if not (out.is_contiguous() and pcm.is_contiguous() and status.is_contiguous()) or out.shape[1] < T or \
                pcm.shape[1] < T:
            raise ValueError("out / pcm / status must be contiguous and hold %d frames per bus" % T)
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the mixer writes them
        bank.join()            # the demodulators that write the plane, before the mixer reads it
        got = self.process_device(bank.audio_device_ptr(), KQ_MON_F32, bank.max_blocks * 2 * olen, 2 * olen, olen, nb,
                                  out.data_ptr(), 2 * out.shape[1], pcm.data_ptr(), 2 * pcm.shape[1], status.data_ptr())
        assert got == T
        # torch's stream waits for the mix, so a later use or reuse of the buffers there comes after it.  (No
        # record_stream on the bank's stream: the allocator would record on it when the tensors are freed, perhaps after
        # the bank that owns the stream has destroyed it.)
        cur.wait_stream(ext)
        return T, out[:, :T], pcm[:, :T], status

    def sync(self):
        self._chk(self.lib.kq_mon_sync(self.h), "kq_mon_sync")

    def reset(self):
        self._chk(self.lib.kq_mon_reset(self.h), "kq_mon_reset")
        self.n = 0


def status_array(st):
    """a status tensor / int32 array [..][5] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


def pcm_array(pcm):
    """a pcm tensor / int16 array of network-order words from process_bank / process_device in host byte order"""
    a = pcm.cpu().numpy() if hasattr(pcm, "cpu") else np.asarray(pcm)
    return np.ascontiguousarray(a, np.int16).view(">i2").astype(np.int16)


__all__ = ["MonBank", "MonConfig", "MonParams", "mon_params", "status_array", "pcm_array", "STATUS_DTYPE", "MAX_SESSIONS",
           "MAX_BUSES", "KQ_MON_F32", "KQ_MON_S16BE"]
