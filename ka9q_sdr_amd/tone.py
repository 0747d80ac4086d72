"""Python mirror of the tone signalling decoder bank (include/ka9q_hip.h: kq_tone_*): the audio of voice channels to DTMF
keys and the tones of sequential selective calls, as events, up to 4096 slots on one tone plan.  ctypes over
libka9q_hip.so; there is no CPU path.  selcall.py holds the tone plans, makes test traffic and reads the events.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
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


class ToneBank(EventBank):
    """Up to max_slots decoders on one tone plan: freqs (Hz; the first group's tones, then the second's), groups (one or
    two counts that cover them), blocks of block_len samples at samprate.  selcall.plan_config(plan, Fs) gives the
    keywords for a plan: ToneBank(Fs, max_slots=..., max_samples=..., **plan_config(DTMF, Fs)).  For process_bank, create
    it on the receiver bank's stream: ToneBank.beside(bank, ...)."""
    _destroy = "kq_tone_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_tone", ToneConfig, ToneParams, staticmethod(tone_params), STATUS_DTYPE
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_incs=[C.c_void_p, C.c_size_t])
    _process_more = [C.c_void_p, C.c_size_t]   # powers and their stride

    def __init__(self, samprate, block_len, freqs, groups, max_slots, max_samples, min_ms=16, frac=None, ratio=64,
                 twist=160, min_blocks=2, input_scale=32767.0, max_events=64, device=0, stream=None):
        groups = tuple(groups) + (0,) * (2 - len(groups))
        if len(groups) != 2:
            raise ValueError("one or two groups")
        if frac is None:
            frac = 16 if groups[1] else 64
        f = np.ascontiguousarray(freqs, np.float32)
        self._create(device, samprate, block_len, f.size, f.ctypes.data_as(C.POINTER(C.c_float)), groups[0], groups[1], min_ms,
                     frac, ratio, twist, min_blocks, input_scale, max_slots, max_events, max_samples, stream)
        self.samprate, self.block_len, self.freqs, self.groups = samprate, block_len, f, groups
        self.ntones = int(f.size)
        self.min_ms, self.frac, self.ratio, self.twist, self.min_blocks = min_ms, frac, ratio, twist, min_blocks
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream

    def get_incs(self):
        """inc_t: the phase increments, uint32 [ntones]"""
        v = np.zeros(self.ntones, np.uint32)
        assert self._call("get_incs", v.ctypes.data, self.ntones) == self.ntones
        return v

    def process(self, x, nblocks=1, fmt=KQ_PCM_F32):
        """as SlotBank.process.  Returns (status, powers): STATUS_DTYPE [max_slots] and uint64 [max_slots][ntones + 1], the
        P_t and E of each slot's last completed block (rows of empty slots 0)."""
        pw = np.zeros((self.max_slots, self.ntones + 1), np.uint64)
        return super().process(x, nblocks, fmt, (pw.ctypes.data, self.ntones + 1)), pw

    def process_device(self, src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr=None, status_stride=1,
                       powers_ptr=None, powers_stride=0, fmt=KQ_PCM_F32, _more=None):
        """asynchronous on the handle's stream; every pointer is device memory"""
        super().process_device(src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr, status_stride, fmt,
                               _more or (powers_ptr, powers_stride))

    def _bank_more(self, torch, powers=None):
        if powers is not None and (not powers.is_contiguous() or powers.dtype != torch.int64
                                   or powers.shape != (self.max_slots, self.ntones + 1)):
            raise ValueError("powers must be a contiguous int64 [max_slots][%d]" % (self.ntones + 1))
        return powers.data_ptr() if powers is not None else None, self.ntones + 1

    def process_bank(self, bank, status=None, powers=None):
        """as SlotBank.process_bank; powers: a torch device tensor int64 [max_slots][ntones + 1] to write (the values are
        unsigned, below 2^55), or None for none.  Returns status."""
        return super().process_bank(bank, status, powers=powers)


def _bind(L):
    return ToneBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return ToneBank.status_array(st)


__all__ = ["ToneBank", "ToneConfig", "ToneParams", "tone_params", "status_array", "Event", "STATUS_DTYPE", "STATUS_WORDS",
           "EVENT_DTYPE", "MAX_SLOTS", "MAX_TONES", "TABLE"]
