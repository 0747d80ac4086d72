"""Python mirror of the ALE decoder bank (include/ka9q_hip.h: kq_ale_*): the audio of USB channels that carry second-generation
ALE (MIL-STD-188-141 Appendix A, 8-FSK at 125 symbols a second) to 24-bit words, as events, up to 16384 slots, each on one
source row with its own tone plan.  ctypes over libka9q_hip.so; there is no CPU path.  ale2g.py holds the word, the Golay
code and the addresses, makes test traffic and reads the events as (preamble, address) pairs.  The signal format there and
here is written down from memory, and the Golay table is not verified against the standard (see ale2g.py).
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import EventBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 16384
TABLE = 1024
TONES = 8
EARLY, CENTRE, LATE = 0, 1, 2
STATUS_DTYPE = np.dtype([("frames", np.uint32), ("ph", np.uint32), ("t", np.int32), ("sym", np.uint32), ("nsym", np.uint32),
                         ("sync_at", np.uint32), ("wpos", np.uint32), ("synced", np.uint32), ("bad", np.uint32),
                         ("events", np.uint32), ("dropped", np.uint32), ("reserved", np.uint32), ("sig", np.uint64),
                         ("nse", np.uint64), ("ee", np.uint64), ("el", np.uint64), ("pe", np.uint64), ("pc", np.uint64),
                         ("oth", np.uint64), ("r0", np.uint64), ("r1", np.uint64), ("r2", np.uint64),
                         ("sum", np.int32, (TONES, 2)), ("acc", np.int64, (TONES, 2))])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
EVENT_DTYPE = np.dtype([("word", np.uint32), ("flags", np.uint32), ("err_a", np.uint32), ("err_b", np.uint32),
                        ("split", np.uint32), ("reserved", np.uint32), ("end_sample", np.uint64), ("sig", np.uint64),
                        ("nse", np.uint64)])

Event = collections.namedtuple("Event", "word flags err_a err_b split reserved end_sample sig nse")
Slot = collections.namedtuple("Slot", "inc tb W")


class AleConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("block_len", C.c_uint), ("warm", C.c_uint), ("snr", C.c_uint),
                ("min_p", C.c_uint64), ("input_scale", C.c_float), ("max_slots", C.c_uint), ("max_events", C.c_uint),
                ("max_samples", C.c_size_t), ("stream", C.c_void_p), ("acq_err", C.c_uint), ("lose", C.c_uint)]


class AleParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("f0", C.c_float), ("df", C.c_float), ("baud", C.c_float)]


class AleSlot(C.Structure):
    _fields_ = [("inc", C.c_uint32 * TONES), ("tb", C.c_uint32), ("W", C.c_uint32)]


def ale_params(source=0, f0=750.0, df=250.0, baud=125.0):
    """kq_ale_params"""
    return AleParams(source, f0, df, baud)


class AleBank(EventBank):
    """Up to max_slots ALE decoders on frames of block_len samples at samprate.  ale2g.ale_config(fs) gives the frame for a
    sample rate: AleBank(fs, max_slots=..., max_samples=..., **ale_config(fs)).  For process_bank, create it on the receiver
    bank's stream: AleBank.beside(bank, ...).  set() touches no device: the next call does."""
    _destroy = "kq_ale_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_ale", AleConfig, AleParams, staticmethod(ale_params), STATUS_DTYPE
    _article = "an"
    _event_dtype, _event = EVENT_DTYPE, Event
    _entry = dict(EventBank._entry, get_slot=[C.c_uint, C.c_void_p])

    def __init__(self, samprate, block_len, max_slots, max_samples, warm=64, snr=80, min_p=1 << 16, input_scale=32767.0,
                 max_events=256, acq_err=1, lose=2, device=0, stream=None):
        self._create(device, samprate, block_len, warm, snr, min_p, input_scale, max_slots, max_events, max_samples, stream,
                     acq_err, lose)
        self.samprate, self.block_len, self.warm, self.snr, self.min_p = samprate, block_len, warm, snr, min_p
        self.input_scale, self.max_slots, self.max_events, self.max_samples = input_scale, max_slots, max_events, max_samples
        self.acq_err, self.lose, self.device, self.stream = acq_err, lose, device, stream

    def get_slot(self, slot):
        """the slot's eight phase increments, symbol length and window: a Slot (inc, tb, W)"""
        v = AleSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(tuple(v.inc), v.tb, v.W)


def _bind(L):
    return AleBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return AleBank.status_array(st)


__all__ = ["AleBank", "AleConfig", "AleParams", "AleSlot", "ale_params", "status_array", "Event", "Slot", "STATUS_DTYPE",
           "STATUS_WORDS", "EVENT_DTYPE", "MAX_SLOTS", "TABLE", "TONES", "EARLY", "CENTRE", "LATE"]
