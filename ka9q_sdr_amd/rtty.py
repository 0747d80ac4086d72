"""Python mirror of the RTTY decoder bank (include/ka9q_hip.h: kq_rtty_*): the audio of SSB channels that carry start-stop
FSK to characters, as events, up to 16384 slots, each on one source row at its own mark and space frequency, baud rate and
character length.  ctypes over libka9q_hip.so; there is no CPU path.  baudot.py holds the alphabet and the shift state,
makes test traffic and reads the events as text.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
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


class RttyBank(EventBank):
    """Up to max_slots RTTY decoders on frames of block_len samples at samprate.  baudot.rtty_config(fs, baud) gives the
    frame for a baud rate: RttyBank(fs, max_slots=..., max_samples=..., **rtty_config(fs, 45.45)).  For process_bank, create
    it on the receiver bank's stream: RttyBank.beside(bank, ...).  set() touches no device: the next call does."""
    _destroy = "kq_rtty_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_rtty", RttyConfig, RttyParams, staticmethod(rtty_params), STATUS_DTYPE
    _event_dtype, _event, _article = EVENT_DTYPE, Event, "an"
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=96, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream

    def get_slot(self, slot):
        """the slot's phase increments, bit length and window: a Slot (inc_m, inc_s, tb, W)"""
        v = RttySlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(v.inc_m, v.inc_s, v.tb, v.W)


def _bind(L):
    return RttyBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return RttyBank.status_array(st)


__all__ = ["RttyBank", "RttyConfig", "RttyParams", "RttySlot", "rtty_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "WAIT", "IDLE", "CHAR"]
