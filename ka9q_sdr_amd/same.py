"""Python mirror of the EAS / SAME decoder bank (include/ka9q_hip.h: kq_same_*): the audio of broadcast and weather-radio
channels that carry Emergency Alert System headers (AFSK at 520.83 bit/s, 2083.3 / 1562.5 Hz) to one event per burst start,
per byte and per burst end, up to 16384 slots, each on one source row.  ctypes over libka9q_hip.so; there is no CPU path.
eas.py builds and parses the header, makes test audio, reads the events into bursts and votes two of three over them.  The
signal format there and here is written down from memory and has met no signal off the air.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
EARLY, CENTRE, LATE = 0, 1, 2
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("ph", np.uint32), ("t", np.int32), ("bit", np.uint32),
                         ("synced", np.uint32), ("bitpos", np.uint32), ("nbytes", np.uint32), ("bad_run", np.uint32),
                         ("plus", np.uint32), ("dashes", np.uint32), ("events", np.uint32), ("dropped", np.uint32),
                         ("syncs", np.uint32), ("eoms", np.uint32), ("complete", np.uint32), ("lost", np.uint32),
                         ("truncated", np.uint32), ("sync_sample", np.uint64), ("sig", np.uint64), ("nse", np.uint64),
                         ("ee", np.uint64), ("el", np.uint64), ("ec", np.uint64), ("pe", np.uint64), ("hi", np.uint64),
                         ("lo", np.uint64), ("r", np.uint64), ("sum", np.int32, (2, 2)), ("acc", np.int64, (2, 2))],
                        align=True)
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("code", np.uint32), ("flags", np.uint32), ("index", np.uint32), ("errs", np.uint32),
                        ("end_sample", np.uint64), ("sig", np.uint64), ("nse", np.uint64)])

Event = collections.namedtuple("Event", "code flags index errs end_sample sig nse")
Slot = collections.namedtuple("Slot", "inc_m inc_s tb W")


class SameConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p), ("sync_errs", C.c_uint), ("lose", C.c_uint),
                ("max_len", C.c_uint)]


class SameParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("mark", C.c_float), ("space", C.c_float), ("baud", C.c_float)]


class SameSlot(C.Structure):
    _fields_ = [("inc_m", C.c_uint32), ("inc_s", C.c_uint32), ("tb", C.c_uint32), ("W", C.c_uint32)]


def same_params(source=0, mark=6250.0 / 3.0, space=1562.5, baud=3125.0 / 6.0):
    """kq_same_params"""
    return SameParams(source, mark, space, baud)


class SameBank(EventBank):
    """Up to max_slots SAME decoders on frames of block_len samples at samprate.  eas.same_config(fs) gives the frame for a
    sample rate: SameBank(fs, max_slots=..., max_samples=..., **same_config(fs)).  For process_bank, create it on the
    receiver bank's stream: SameBank.beside(bank, ...).  set() touches no device: the next call does.  An alert is some 150
    to 760 events: clear_events() once they are read."""
    _destroy = "kq_same_destroy"
    _prefix, _config, _params, _make_params, _status = ("kq_same", SameConfig, SameParams, staticmethod(same_params),
                                                         STATUS_DTYPE)
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=64, min_p=1 << 16, input_scale=32767.0,
                 max_events=1024, sync_errs=2, lose=3, max_len=248, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream,
                     sync_errs, lose, max_len)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.sync_errs, self.lose, self.max_len, self.device, self.stream = sync_errs, lose, max_len, device, stream

    def get_slot(self, slot):
        """the slot's phase increments, bit length and window: a Slot (inc_m, inc_s, tb, W)"""
        v = SameSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(v.inc_m, v.inc_s, v.tb, v.W)


def _bind(L):
    return SameBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return SameBank.status_array(st)


__all__ = ["SameBank", "SameConfig", "SameParams", "SameSlot", "same_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "EARLY", "CENTRE", "LATE", "KQ_PCM_F32", "KQ_PCM_S16BE"]
