"""Python mirror of the CW (Morse) decoder bank (include/ka9q_hip.h: kq_cw_*): the audio of CW channels to characters, as
events, up to 16384 slots, each on one source row at one pitch.  ctypes over libka9q_hip.so; there is no CPU path.
morse.py holds the alphabet, makes test traffic and reads the events as text.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("key", np.uint32), ("run", np.uint32), ("unit", np.uint32),
                         ("events", np.uint32), ("dropped", np.uint32), ("cand", np.uint32), ("code", np.uint32),
                         ("nelem", np.uint32), ("flags", np.uint32), ("hi", np.uint64), ("lo", np.uint64),
                         ("first", np.uint64), ("last", np.uint64), ("acc_i", np.int64), ("acc_q", np.int64)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("code", np.uint32), ("nelem", np.uint32), ("unit", np.uint32), ("reserved", np.uint32),
                        ("start_sample", np.uint64), ("end_sample", np.uint64), ("peak", np.uint64)])

Event = collections.namedtuple("Event", "code nelem unit start_sample end_sample peak")


class CwConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("min_wpm", C.c_float),
                ("max_wpm", C.c_float), ("deb", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint), ("min_p", C.c_uint64),
                ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class CwParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("pitch", C.c_float), ("wpm", C.c_float)]


def cw_params(source=0, pitch=700.0, wpm=20.0):
    """kq_cw_params"""
    return CwParams(source, pitch, wpm)


class CwBank(EventBank):
    """Up to max_slots Morse decoders on frames of block_len samples at samprate, following speeds of min_wpm to max_wpm.
    morse.cw_config(fs, max_wpm) gives the keywords for a top speed: CwBank(fs, max_slots=..., max_samples=...,
    **cw_config(fs, 60)).  For process_bank, create it on the receiver bank's stream: CwBank.beside(bank, ...).  set()
    touches no device: the next call does."""
    _destroy = "kq_cw_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_cw", CwConfig, CwParams, staticmethod(cw_params), STATUS_DTYPE
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_inc=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, min_wpm=5.0, max_wpm=60.0, deb=2, warm=64, snr=256,
                 min_p=1 << 16, input_scale=32767.0, max_events=256, device=0, stream=None):
        self._create(device, samprate, block_len, min_wpm, max_wpm, deb, warm, snr, min_p, input_scale, max_slots, max_events,
                     max_samples, stream)
        self.samprate, self.block_len, self.min_wpm, self.max_wpm = samprate, block_len, min_wpm, max_wpm
        self.deb, self.warm, self.snr, self.min_p = deb, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.device, self.stream = device, stream

    def get_inc(self, slot):
        """the slot's phase increment"""
        v = np.zeros(1, np.uint32)
        self._call("get_inc", slot, v.ctypes.data)
        return int(v[0])


def _bind(L):
    return CwBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return CwBank.status_array(st)


__all__ = ["CwBank", "CwConfig", "CwParams", "cw_params", "status_array", "Event", "STATUS_DTYPE", "STATUS_WORDS",
           "EVENT_DTYPE", "MAX_SLOTS", "TABLE"]
