"""Python mirror of the NAVTEX decoder bank (include/ka9q_hip.h: kq_navtex_*): the audio of SSB channels that carry NAVTEX
or SITOR-B broadcasts (CCIR 476 collective B mode, 2-FSK at 100 baud) to one event per character, up to 16384 slots, each on
one source row at its own tone pair.  ctypes over libka9q_hip.so; there is no CPU path.  ccir476.py holds the alphabet, the
interleave, makes test traffic, and turns the events into text and ZCZC .. NNNN messages.  The signal format and the
alphabet there and here are written down from memory and have met no signal off the air (ccir476.py says what is held by a
test and what is not).
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
EARLY, CENTRE, LATE = 0, 1, 2
DX, RX = 0, 1
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("ph", np.uint32), ("t", np.int32), ("bit", np.uint32), ("nbits", np.uint32),
                         ("synced", np.uint32), ("bitpos", np.uint32), ("kind", np.uint32), ("inverted", np.uint32),
                         ("run", np.uint32), ("events", np.uint32), ("dropped", np.uint32), ("syncs", np.uint32),
                         ("tsyncs", np.uint32), ("losses", np.uint32), ("idles", np.uint32), ("sig", np.uint64),
                         ("nse", np.uint64), ("ee", np.uint64), ("el", np.uint64), ("ec", np.uint64), ("pe", np.uint64),
                         ("hi", np.uint64), ("lo", np.uint64), ("r_hi", np.uint64), ("r_lo", np.uint64),
                         ("sum", np.int32, (2, 2)), ("acc", np.int64, (2, 2))])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("code", np.uint32), ("flags", np.uint32), ("dx", np.uint32), ("rx", np.uint32), ("end_sample", np.uint64),
                        ("sig", np.uint64), ("nse", np.uint64)])

Event = collections.namedtuple("Event", "code flags dx rx end_sample sig nse")
Slot = collections.namedtuple("Slot", "inc_m inc_s tb W")


class NavtexConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p), ("acq", C.c_uint), ("pairs", C.c_uint), ("lose", C.c_uint)]


class NavtexParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("mark", C.c_float), ("space", C.c_float), ("baud", C.c_float)]


class NavtexSlot(C.Structure):
    _fields_ = [("inc_m", C.c_uint32), ("inc_s", C.c_uint32), ("tb", C.c_uint32), ("W", C.c_uint32)]


def navtex_params(source=0, mark=1785.0, space=1615.0, baud=100.0):
    """kq_navtex_params"""
    return NavtexParams(source, mark, space, baud)


class NavtexBank(EventBank):
    """Up to max_slots NAVTEX decoders on frames of block_len samples at samprate.  ccir476.navtex_config(fs) gives the
    frame for a sample rate: NavtexBank(fs, max_slots=..., max_samples=..., **navtex_config(fs)).  For process_bank, create
    it on the receiver bank's stream: NavtexBank.beside(bank, ...).  set() touches no device: the next call does.  An arena
    takes seven characters a second: clear_events() once they are read."""
    _destroy = "kq_navtex_destroy"
    _prefix, _config, _params, _make_params, _status = ("kq_navtex", NavtexConfig, NavtexParams, staticmethod(navtex_params),
                                                         STATUS_DTYPE)
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=64, min_p=1 << 16, input_scale=32767.0,
                 max_events=512, acq=4, pairs=4, lose=16, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream,
                     acq, pairs, lose)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.acq, self.pairs, self.lose, self.device, self.stream = acq, pairs, lose, device, stream

    def get_slot(self, slot):
        """the slot's phase increments, bit length and window: a Slot (inc_m, inc_s, tb, W)"""
        v = NavtexSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(v.inc_m, v.inc_s, v.tb, v.W)


def _bind(L):
    return NavtexBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return NavtexBank.status_array(st)


__all__ = ["NavtexBank", "NavtexConfig", "NavtexParams", "NavtexSlot", "navtex_params", "status_array", "Event", "Slot",
           "STATUS_DTYPE", "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "EARLY", "CENTRE", "LATE", "DX", "RX",
           "KQ_PCM_F32", "KQ_PCM_S16BE"]
