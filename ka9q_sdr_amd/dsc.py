"""Python mirror of the DSC decoder bank (include/ka9q_hip.h: kq_dsc_*): the audio of SSB channels (or of a flat FM channel
at 96 kHz) that carry GMDSS digital selective calling (ITU-R M.493, 2-FSK at 100 or 1200 baud) to whole messages, as
events, up to 16384 slots, each on one source row at its own tone pair and baud rate.  ctypes over libka9q_hip.so; there
is no CPU path.  itu493.py holds the symbol, the sequence and three kinds of message, makes test traffic and reads the
events.  The signal format there and here is written down from memory and has met no signal off the air (see itu493.py).
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
MAX_SYMBOLS = 64
EARLY, CENTRE, LATE = 0, 1, 2
# kq_dsc_status with kq_dsc_message, its last member, written out flat
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("ph", np.uint32), ("t", np.int32), ("bit", np.uint32), ("nbits", np.uint32),
                         ("synced", np.uint32), ("bitpos", np.uint32), ("events", np.uint32), ("dropped", np.uint32),
                         ("syncs", np.uint32), ("aborted", np.uint32), ("reserved", np.uint32), ("sig", np.uint64),
                         ("nse", np.uint64), ("ee", np.uint64), ("el", np.uint64), ("ec", np.uint64), ("pe", np.uint64),
                         ("hi", np.uint64), ("lo", np.uint64), ("r", np.uint64), ("sum", np.int32, (2, 2)), ("acc", np.int64, (2, 2)),
                         ("inverted", np.uint32), ("place", np.uint32), ("nsym", np.uint32), ("nres", np.uint32),
                         ("holes", np.uint32), ("from_rx", np.uint32), ("run", np.uint32), ("ecc", np.uint32), ("eos", np.uint32),
                         ("reserved2", np.uint32), ("hole_mask", np.uint64), ("sync_sample", np.uint64),
                         ("msg", np.uint8, (MAX_SYMBOLS,))])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("sym", np.uint8, (MAX_SYMBOLS,)), ("nsym", np.uint32), ("flags", np.uint32), ("holes", np.uint32),
                        ("from_rx", np.uint32), ("hole_mask", np.uint64), ("sync_sample", np.uint64), ("end_sample", np.uint64),
                        ("sig", np.uint64), ("nse", np.uint64)])

Event = collections.namedtuple("Event", "sym nsym flags holes from_rx hole_mask sync_sample end_sample sig nse")   # sym: bytes
Slot = collections.namedtuple("Slot", "inc_m inc_s tb W")


class DscConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p), ("acq", C.c_uint), ("lose", C.c_uint)]


class DscParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("mark", C.c_float), ("space", C.c_float), ("baud", C.c_float)]


class DscSlot(C.Structure):
    _fields_ = [("inc_m", C.c_uint32), ("inc_s", C.c_uint32), ("tb", C.c_uint32), ("W", C.c_uint32)]


def dsc_params(source=0, mark=1785.0, space=1615.0, baud=100.0):
    """kq_dsc_params"""
    return DscParams(source, mark, space, baud)


class DscBank(EventBank):
    """Up to max_slots DSC decoders on frames of block_len samples at samprate.  itu493.dsc_config(fs, baud) gives the
    frame for a sample rate: DscBank(fs, max_slots=..., max_samples=..., **dsc_config(fs)).  For process_bank, create it on
    the receiver bank's stream: DscBank.beside(bank, ...).  set() touches no device: the next call does."""
    _destroy = "kq_dsc_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_dsc", DscConfig, DscParams, staticmethod(dsc_params), STATUS_DTYPE
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=64, min_p=1 << 16, input_scale=32767.0,
                 max_events=64, acq=2, lose=3, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream,
                     acq, lose)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.acq, self.lose, self.device, self.stream = acq, lose, device, stream

    def event(self, slot, index):
        """one event of a slot's arena, an Event whose sym is the 64 bytes; synchronous"""
        r = np.zeros(1, self._event_dtype)
        self._call("pull_event", slot, index, r.ctypes.data)
        return Event(r[0]["sym"].tobytes(), *(int(r[0][k]) for k in Event._fields[1:]))

    def get_slot(self, slot):
        """the slot's phase increments, bit length and window: a Slot (inc_m, inc_s, tb, W)"""
        v = DscSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(v.inc_m, v.inc_s, v.tb, v.W)


def _bind(L):
    return DscBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return DscBank.status_array(st)


__all__ = ["DscBank", "DscConfig", "DscParams", "DscSlot", "dsc_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "MAX_SYMBOLS", "EARLY", "CENTRE", "LATE"]
