"""Python mirror of the tone signalling decoder bank (include/ka9q_hip.h: kq_tone_*): the audio of voice channels to DTMF
keys and the tones of sequential selective calls, as events, up to 4096 slots on one tone plan.  ctypes over
libka9q_hip.so; there is no CPU path.  selcall.py holds the tone plans, makes test traffic and reads the events.
"""
import collections
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 4096
MAX_TONES = 32
TABLE = 1024
STATUS_DTYPE = np.dtype([("blocks", np.uint32), ("valid_blocks", np.uint32), ("events", np.uint32), ("dropped", np.uint32),
                         ("cur", np.int32), ("run", np.uint32), ("energy", np.uint64)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("symbol", np.int32), ("blocks", np.uint32), ("start_sample", np.uint64), ("peak", np.uint64)])

Event = collections.namedtuple("Event", "symbol blocks start_sample peak")


class ToneConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("ntones", C.c_uint),
                ("freqs", C.POINTER(C.c_float)), ("group0", C.c_uint), ("group1", C.c_uint), ("min_ms", C.c_uint),
                ("frac", C.c_uint), ("ratio", C.c_uint), ("twist", C.c_uint), ("min_blocks", C.c_uint),
                ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class ToneParams(C.Structure):
    _fields_ = [("source", C.c_uint)]


def tone_params(source=0):
    """kq_tone_params"""
    return ToneParams(source)


def _bind(L):
    if getattr(L, "_kq_tone_bound", False):
        return L
    L.kq_tone_create.restype = C.c_void_p
    L.kq_tone_create.argtypes = [C.POINTER(ToneConfig)]
    L.kq_tone_destroy.argtypes = [C.c_void_p]
    L.kq_tone_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(ToneParams)]
    L.kq_tone_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_tone_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int,
                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.kq_tone_pull_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.kq_tone_pull_event.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    L.kq_tone_clear_events.argtypes = [C.c_void_p]
    L.kq_tone_get_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_tone_get_incs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_tone_sync.argtypes = [C.c_void_p]
    L.kq_tone_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_tone_bound = True
    return L


class ToneBank(Handle):
    """Up to max_slots decoders on one tone plan: freqs (Hz; the first group's tones, then the second's), groups (one or
    two counts that cover them), blocks of block_len samples at samprate.  selcall.plan_config(plan, Fs) gives the
    keywords for a plan: ToneBank(Fs, max_slots=..., max_samples=..., **plan_config(DTMF, Fs)).  For process_bank, create
    it on the receiver bank's stream: ToneBank.beside(bank, ...)."""
    _destroy = "kq_tone_destroy"

    def __init__(self, samprate, block_len, freqs, groups, max_slots, max_samples, min_ms=16, frac=None, ratio=64,
                 twist=160, min_blocks=2, input_scale=32767.0, max_events=64, device=0, stream=None):
        self.lib = _bind(load_library())
        groups = tuple(groups) + (0,) * (2 - len(groups))
        if len(groups) != 2:
            raise ValueError("one or two groups")
        if frac is None:
            frac = 16 if groups[1] else 64
        f = np.ascontiguousarray(freqs, np.float32)
        cfg = ToneConfig(device, samprate, block_len, f.size, f.ctypes.data_as(C.POINTER(C.c_float)), groups[0], groups[1],
                         min_ms, frac, ratio, twist, min_blocks, input_scale, max_slots, max_events, max_samples, stream)
        self.h = self.lib.kq_tone_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_tone_create: " + _err(self.lib))
        self.samprate, self.block_len, self.freqs, self.groups = samprate, block_len, f, groups
        self.ntones = int(f.size)
        self.min_ms, self.frac, self.ratio, self.twist, self.min_blocks = min_ms, frac, ratio, twist, min_blocks
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream
        self.n = 0   # samples taken so far

    @classmethod
    def beside(cls, bank, block_len, freqs, groups, max_slots, **kw):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D)"""
        lib = _bind(load_library())
        return cls(bank.samprate / bank.D, block_len, freqs, groups, max_slots, bank.max_blocks * bank.olen,
                   stream=lib.kq_bank_stream(bank.h), **kw)

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (a ToneParams, or tone_params() keywords); it starts cold at the next call"""
        p = params if params is not None else tone_params(**kw)
        self._chk(self.lib.kq_tone_set(self.h, slot, C.byref(p)), "kq_tone_set")

    def remove(self, slot):
        self._chk(self.lib.kq_tone_remove(self.h, slot), "kq_tone_remove")

    def get_table(self):
        """C: the cosine table, int16 [1024]"""
        c = np.zeros(TABLE, np.int16)
        assert self._chk(self.lib.kq_tone_get_table(self.h, c.ctypes.data, TABLE), "kq_tone_get_table") == TABLE
        return c

    def get_incs(self):
        """inc_t: the phase increments, uint32 [ntones]"""
        v = np.zeros(self.ntones, np.uint32)
        assert self._chk(self.lib.kq_tone_get_incs(self.h, v.ctypes.data, self.ntones), "kq_tone_get_incs") == self.ntones
        return v

    def process(self, x, nblocks=1, fmt=KQ_PCM_F32):
        """x: host [rows][n] (row = source), float32, or for KQ_PCM_S16BE int16 values that go out in network byte order; n
        split into nblocks equal blocks.  Synchronous.  Returns (status, powers): STATUS_DTYPE [max_slots] and uint64
        [max_slots][ntones + 1], the P_t and E of each slot's last completed block (rows of empty slots 0)."""
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x, ">i2" if fmt == KQ_PCM_S16BE else np.float32)
        n = x.shape[1]
        if n % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (n, nblocks))
        st = np.zeros(self.max_slots, STATUS_DTYPE)
        pw = np.zeros((self.max_slots, self.ntones + 1), np.uint64)
        self._chk(self.lib.kq_tone_process(self.h, x.ctypes.data, fmt, n, n // nblocks, n // nblocks, nblocks, 0, st.ctypes.data,
                                           1, pw.ctypes.data, self.ntones + 1), "kq_tone_process")
        self.n += n
        return st, pw

    def process_device(self, src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr=None, status_stride=1,
                       powers_ptr=None, powers_stride=0, fmt=KQ_PCM_F32):
        """asynchronous on the handle's stream; every pointer is device memory"""
        self._chk(self.lib.kq_tone_process(self.h, src_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, status_ptr,
                                           status_stride, powers_ptr, powers_stride), "kq_tone_process")
        self.n += block_len * nblocks

    def process_bank(self, bank, status=None, powers=None):
        """Decode a receiver Bank's last call straight from its device audio plane on the bank's stream, with no host round
        trip and no host wait: kq_bank_join first orders the decode behind the bank's demodulators.  status: a contiguous
        torch device tensor int32 [max_slots][STATUS_WORDS] to write, or None for a new zeroed one (status_array() views
        it as STATUS_DTYPE); powers: int64 [max_slots][ntones + 1] (the values are unsigned, below 2^55), or None for
        none.  Returns status.  The decode waits for what torch's current stream has queued, and that stream waits for
        the decode."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs a ToneBank on the bank's stream (ToneBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        dev = torch.device("cuda", self.device)
        if status is None:
            status = torch.zeros((self.max_slots, STATUS_WORDS), dtype=torch.int32, device=dev)
        if not status.is_contiguous() or status.shape != (self.max_slots, STATUS_WORDS):
            raise ValueError("status must be a contiguous int32 [max_slots][%d]" % STATUS_WORDS)
        if powers is not None and (not powers.is_contiguous() or powers.dtype != torch.int64
                                   or powers.shape != (self.max_slots, self.ntones + 1)):
            raise ValueError("powers must be a contiguous int64 [max_slots][%d]" % (self.ntones + 1))
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the decoder writes them
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, status.data_ptr(), 1,
                            powers.data_ptr() if powers is not None else None, self.ntones + 1)
        cur.wait_stream(ext)
        return status

    def counts(self):
        """events in every slot's arena, uint32 [max_slots]; synchronous"""
        c = np.zeros(self.max_slots, np.uint32)
        self._chk(self.lib.kq_tone_pull_counts(self.h, c.ctypes.data), "kq_tone_pull_counts")
        return c

    def event(self, slot, index):
        """one event of a slot's arena, an Event (symbol, blocks, start_sample, peak); synchronous"""
        r = np.zeros(1, EVENT_DTYPE)
        self._chk(self.lib.kq_tone_pull_event(self.h, slot, index, r.ctypes.data), "kq_tone_pull_event")
        return Event(*(int(v) for v in r[0]))

    def events(self, slot, count=None):
        """every event of a slot's arena, in order"""
        if count is None:
            count = int(self.counts()[slot])
        return [self.event(slot, k) for k in range(count)]

    def clear_events(self):
        self._chk(self.lib.kq_tone_clear_events(self.h), "kq_tone_clear_events")

    def sync(self):
        self._chk(self.lib.kq_tone_sync(self.h), "kq_tone_sync")

    def reset(self):
        self._chk(self.lib.kq_tone_reset(self.h), "kq_tone_reset")
        self.n = 0


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


__all__ = ["ToneBank", "ToneConfig", "ToneParams", "tone_params", "status_array", "Event", "STATUS_DTYPE", "STATUS_WORDS",
           "EVENT_DTYPE", "MAX_SLOTS", "MAX_TONES", "TABLE"]
