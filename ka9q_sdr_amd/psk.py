"""Python mirror of the PSK decoder bank (include/ka9q_hip.h: kq_psk_*): the audio of SSB channels that carry PSK31, PSK63
or PSK125 to characters, as events, up to 16384 slots, each on one source row at its own pitch and baud rate.  ctypes over
libka9q_hip.so; there is no CPU path.  varicode.py holds the alphabet, makes test traffic, reads the events as text and
turns an event's rotation into a frequency offset.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
EARLY, CENTRE, LATE = 0, 1, 2
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("ph", np.uint32), ("t", np.int32), ("shreg", np.uint32), ("over", np.uint32),
                         ("events", np.uint32), ("dropped", np.uint32), ("reserved", np.uint32), ("sig", np.uint64),
                         ("qre", np.uint64), ("qim", np.uint64), ("ee", np.uint64), ("el", np.uint64), ("pe", np.uint64),
                         ("pc", np.uint64), ("rot_r", np.int64), ("rot_i", np.int64), ("cr", np.int32), ("ci", np.int32),
                         ("pr", np.int32), ("pi", np.int32), ("sum_i", np.int32), ("sum_q", np.int32), ("acc_i", np.int64),
                         ("acc_q", np.int64)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("code", np.uint32), ("flags", np.uint32), ("end_sample", np.uint64), ("sig", np.uint64),
                        ("rot_r", np.int32), ("rot_i", np.int32)])

Event = collections.namedtuple("Event", "code flags end_sample sig rot_r rot_i")
Slot = collections.namedtuple("Slot", "inc tb W")


class PskConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class PskParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("pitch", C.c_float), ("baud", C.c_float)]


class PskSlot(C.Structure):
    _fields_ = [("inc", C.c_uint32), ("tb", C.c_uint32), ("W", C.c_uint32), ("reserved", C.c_uint32)]


def psk_params(source=0, pitch=1000.0, baud=31.25):
    """kq_psk_params"""
    return PskParams(source, pitch, baud)


class PskBank(EventBank):
    """Up to max_slots PSK decoders on frames of block_len samples at samprate.  varicode.psk_config(fs, baud) gives the
    frame for a baud rate: PskBank(fs, max_slots=..., max_samples=..., **psk_config(fs, 31.25)).  For process_bank, create
    it on the receiver bank's stream: PskBank.beside(bank, ...).  set() touches no device: the next call does."""
    _destroy = "kq_psk_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_psk", PskConfig, PskParams, staticmethod(psk_params), STATUS_DTYPE
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=32, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream

    def get_slot(self, slot):
        """the slot's phase increment, symbol length and window: a Slot (inc, tb, W)"""
        v = PskSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(v.inc, v.tb, v.W)


def _bind(L):
    return PskBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return PskBank.status_array(st)


__all__ = ["PskBank", "PskConfig", "PskParams", "PskSlot", "psk_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "EARLY", "CENTRE", "LATE"]
