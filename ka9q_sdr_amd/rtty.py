"""Python mirror of the RTTY decoder bank (include/ka9q_hip.h: kq_rtty_*): the audio of SSB channels that carry start-stop
FSK to characters, as events, up to 16384 slots, each on one source row at its own mark and space frequency, baud rate and
character length.  ctypes over libka9q_hip.so; there is no CPU path.  baudot.py holds the alphabet and the shift state,
makes test traffic and reads the events as text.
"""
import collections
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
WAIT, IDLE, CHAR = 0, 1, 2
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("state", np.uint32), ("bit", np.int32), ("code", np.uint32), ("t", np.int32),
                         ("events", np.uint32), ("dropped", np.uint32), ("ferr", np.uint32), ("false_starts", np.uint32),
                         ("reserved", np.uint32), ("sig", np.uint64), ("nse", np.uint64), ("start", np.uint64),
                         ("sum_im", np.int32), ("sum_qm", np.int32), ("sum_is", np.int32), ("sum_qs", np.int32),
                         ("acc_im", np.int64), ("acc_qm", np.int64), ("acc_is", np.int64), ("acc_qs", np.int64)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("code", np.uint32), ("flags", np.uint32), ("start_sample", np.uint64), ("sig", np.uint64),
                        ("nse", np.uint64)])

Event = collections.namedtuple("Event", "code flags start_sample sig nse")
Slot = collections.namedtuple("Slot", "inc_m inc_s tb W")


class RttyConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class RttyParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("mark", C.c_float), ("space", C.c_float), ("baud", C.c_float), ("nbits", C.c_uint)]


class RttySlot(C.Structure):
    _fields_ = [("inc_m", C.c_uint32), ("inc_s", C.c_uint32), ("tb", C.c_uint32), ("W", C.c_uint32)]


def rtty_params(source=0, mark=2125.0, space=2295.0, baud=45.45, nbits=5):
    """kq_rtty_params"""
    return RttyParams(source, mark, space, baud, nbits)


def _bind(L):
    if getattr(L, "_kq_rtty_bound", False):
        return L
    L.kq_rtty_create.restype = C.c_void_p
    L.kq_rtty_create.argtypes = [C.POINTER(RttyConfig)]
    L.kq_rtty_destroy.argtypes = [C.c_void_p]
    L.kq_rtty_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(RttyParams)]
    L.kq_rtty_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_rtty_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int,
                                  C.c_void_p, C.c_size_t]
    L.kq_rtty_pull_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.kq_rtty_pull_event.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    L.kq_rtty_clear_events.argtypes = [C.c_void_p]
    L.kq_rtty_get_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_rtty_get_slot.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
    L.kq_rtty_sync.argtypes = [C.c_void_p]
    L.kq_rtty_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_rtty_bound = True
    return L


class RttyBank(Handle):
    """Up to max_slots RTTY decoders on frames of block_len samples at samprate.  baudot.rtty_config(fs, baud) gives the
    frame for a baud rate: RttyBank(fs, max_slots=..., max_samples=..., **rtty_config(fs, 45.45)).  For process_bank, create
    it on the receiver bank's stream: RttyBank.beside(bank, ...)."""
    _destroy = "kq_rtty_destroy"

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=96, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, device=0, stream=None):
        self.lib = _bind(load_library())
        cfg = RttyConfig(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream)
        self.h = self.lib.kq_rtty_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_rtty_create: " + _err(self.lib))
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream
        self.n = 0   # samples taken so far

    @classmethod
    def beside(cls, bank, block_len, max_slots, **kw):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D)"""
        lib = _bind(load_library())
        return cls(bank.samprate / bank.D, block_len, max_slots, bank.max_blocks * bank.olen,
                   stream=lib.kq_bank_stream(bank.h), **kw)

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (an RttyParams, or rtty_params() keywords); it starts cold at the next call.  Touches no
        device: the next call does"""
        p = params if params is not None else rtty_params(**kw)
        self._chk(self.lib.kq_rtty_set(self.h, slot, C.byref(p)), "kq_rtty_set")

    def remove(self, slot):
        self._chk(self.lib.kq_rtty_remove(self.h, slot), "kq_rtty_remove")

    def get_table(self):
        """C: the cosine table, int16 [1024]"""
        c = np.zeros(TABLE, np.int16)
        assert self._chk(self.lib.kq_rtty_get_table(self.h, c.ctypes.data, TABLE), "kq_rtty_get_table") == TABLE
        return c

    def get_slot(self, slot):
        """the slot's phase increments, bit length and window: a Slot (inc_m, inc_s, tb, W)"""
        v = RttySlot()
        self._chk(self.lib.kq_rtty_get_slot(self.h, slot, C.byref(v)), "kq_rtty_get_slot")
        return Slot(v.inc_m, v.inc_s, v.tb, v.W)

    def process(self, x, nblocks=1, fmt=KQ_PCM_F32):
        """x: host [rows][n] (row = source), float32, or for KQ_PCM_S16BE int16 values that go out in network byte order; n
        split into nblocks equal blocks.  Synchronous.  Returns status: STATUS_DTYPE [max_slots] (empty slots 0)."""
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x, ">i2" if fmt == KQ_PCM_S16BE else np.float32)
        n = x.shape[1]
        if n % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (n, nblocks))
        st = np.zeros(self.max_slots, STATUS_DTYPE)
        self._chk(self.lib.kq_rtty_process(self.h, x.ctypes.data, fmt, n, n // nblocks, n // nblocks, nblocks, 0,
                                           st.ctypes.data, 1), "kq_rtty_process")
        self.n += n
        return st

    def process_device(self, src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr=None, status_stride=1,
                       fmt=KQ_PCM_F32):
        """asynchronous on the handle's stream; every pointer is device memory"""
        self._chk(self.lib.kq_rtty_process(self.h, src_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, status_ptr,
                                           status_stride), "kq_rtty_process")
        self.n += block_len * nblocks

    def process_bank(self, bank, status=None):
        """Decode a receiver Bank's last call straight from its device audio plane on the bank's stream, with no host round
        trip and no host wait: kq_bank_join first orders the decode behind the bank's demodulators.  status: a contiguous
        torch device tensor int32 [max_slots][STATUS_WORDS] to write, or None for a new zeroed one (status_array() views
        it as STATUS_DTYPE).  Returns status.  The decode waits for what torch's current stream has queued, and that
        stream waits for the decode."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs an RttyBank on the bank's stream (RttyBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        dev = torch.device("cuda", self.device)
        if status is None:
            status = torch.zeros((self.max_slots, STATUS_WORDS), dtype=torch.int32, device=dev)
        if not status.is_contiguous() or status.shape != (self.max_slots, STATUS_WORDS):
            raise ValueError("status must be a contiguous int32 [max_slots][%d]" % STATUS_WORDS)
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the decoder writes them
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, status.data_ptr(), 1)
        cur.wait_stream(ext)
        return status

    def counts(self):
        """events in every slot's arena, uint32 [max_slots]; synchronous"""
        c = np.zeros(self.max_slots, np.uint32)
        self._chk(self.lib.kq_rtty_pull_counts(self.h, c.ctypes.data), "kq_rtty_pull_counts")
        return c

    def event(self, slot, index):
        """one event of a slot's arena, an Event (code, flags, start_sample, sig, nse); synchronous"""
        r = np.zeros(1, EVENT_DTYPE)
        self._chk(self.lib.kq_rtty_pull_event(self.h, slot, index, r.ctypes.data), "kq_rtty_pull_event")
        return Event(*(int(r[0][k]) for k in Event._fields))

    def events(self, slot, count=None):
        """every event of a slot's arena, in order"""
        if count is None:
            count = int(self.counts()[slot])
        return [self.event(slot, k) for k in range(count)]

    def clear_events(self):
        self._chk(self.lib.kq_rtty_clear_events(self.h), "kq_rtty_clear_events")

    def sync(self):
        self._chk(self.lib.kq_rtty_sync(self.h), "kq_rtty_sync")

    def reset(self):
        self._chk(self.lib.kq_rtty_reset(self.h), "kq_rtty_reset")
        self.n = 0


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


__all__ = ["RttyBank", "RttyConfig", "RttyParams", "RttySlot", "rtty_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "WAIT", "IDLE", "CHAR"]
