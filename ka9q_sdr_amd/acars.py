"""Python mirror of the ACARS decoder bank (include/ka9q_hip.h: kq_acars_*): the audio of AM airband channels to ACARS
blocks, up to 4096 slots, each on one source row.  ctypes over libka9q_hip.so; there is no CPU path.  arinc618.py makes
test traffic, parses and repairs the blocks and reads a bank's arenas.
"""
import collections
import ctypes as C

import numpy as np

from ._slotbank import SlotBank
from .arinc618 import Record
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 4096
MAX_BLOCK_BYTES = 256
GOOD, ENDED_BY_ETB, OVERRUN = 1, 2, 4
STATUS_DTYPE = np.dtype([("syncs", np.uint32), ("blocks_good", np.uint32), ("blocks_bad", np.uint32), ("overruns", np.uint32),
                         ("dropped", np.uint32), ("discarded", np.uint32), ("in_block", np.uint32), ("k", np.uint32),
                         ("nbits", np.uint32), ("cur", np.uint32), ("length", np.uint32), ("parity_errors", np.uint32),
                         ("crc", np.uint32), ("ending", np.uint32), ("cnt", np.uint32), ("reserved", np.uint32), ("t", np.int64),
                         ("search_from", np.int64), ("acc", np.int64), ("sync_sample", np.uint64), ("sync_c2", np.uint64),
                         ("sync_e", np.uint64), ("rr", np.int32), ("ri", np.int32)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
INFO_DTYPE = np.dtype([("length", np.uint32), ("flags", np.uint32), ("parity_errors", np.uint32), ("reserved", np.uint32),
                       ("sync_sample", np.uint64), ("end_sample", np.uint64), ("sync_c2", np.uint64), ("sync_e", np.uint64),
                       ("r2", np.uint64)])

Slot = collections.namedtuple("Slot", "source inc taps w e tb history piece")


class AcarsConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("input_scale", C.c_float), ("sync_num", C.c_uint),
                ("sync_den", C.c_uint), ("max_parity_errors", C.c_uint), ("max_block_bytes", C.c_uint), ("max_slots", C.c_uint),
                ("max_blocks", C.c_uint), ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class AcarsParams(C.Structure):
    _fields_ = [("source", C.c_uint)]


class AcarsSlot(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in Slot._fields]


def acars_params(source=0):
    """kq_acars_params"""
    return AcarsParams(source)


class AcarsBank(SlotBank):
    """Up to max_slots ACARS decoders at samprate (9600 to 96000 Hz), each on one row of AM audio.  For process_bank,
    create it on the receiver bank's stream: AcarsBank.beside(bank, ...).  set() touches no device: the next call does.
    arinc618.read_blocks(bank) gives what the arenas hold, parsed."""
    _destroy = "kq_acars_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_acars", AcarsConfig, AcarsParams, staticmethod(acars_params), STATUS_DTYPE
    _article = "an"
    _entry = {"pull_block": [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p], "clear_blocks": [],
              "get_taps": [C.c_void_p, C.c_size_t], "get_slot": [C.c_uint, C.c_void_p]}

    def __init__(self, samprate, max_slots, max_samples, input_scale=32767.0, sync_num=1, sync_den=2, max_parity_errors=3,
                 max_block_bytes=MAX_BLOCK_BYTES, max_blocks=16, device=0, stream=None):
        self._create(device, samprate, input_scale, sync_num, sync_den, max_parity_errors, max_block_bytes, max_slots, max_blocks,
                     max_samples, stream)
        self.samprate, self.input_scale, self.sync_num, self.sync_den = samprate, input_scale, sync_num, sync_den
        self.max_parity_errors, self.max_block_bytes, self.max_blocks = max_parity_errors, max_block_bytes, max_blocks
        self.max_slots, self.max_samples, self.device, self.stream = max_slots, max_samples, device, stream

    def get_taps(self):
        """hq: the matched filter, int16 [FL]"""
        hq = np.zeros(80, np.int16)
        n = self._call("get_taps", hq.ctypes.data, hq.size)
        return hq[:n].copy()

    def get_slot(self, slot):
        """the slot's source and the bank's integers: a Slot"""
        v = AcarsSlot()
        self._call("get_slot", slot, C.byref(v))
        return Slot(*(getattr(v, k) for k in Slot._fields))

    def block(self, slot, index):
        """one block of a slot's arena, an arinc618.Record; synchronous"""
        buf = np.zeros(self.max_block_bytes, np.uint8)
        info = np.zeros(1, INFO_DTYPE)
        n = self._call("pull_block", slot, index, buf.ctypes.data, buf.size, info.ctypes.data)
        r = info[0]
        assert n == int(r["length"])
        return Record(bytes(buf[:n]), n, *(int(r[k]) for k in Record._fields[2:]))

    def blocks(self, slot, count=None):
        """every block of a slot's arena, in order"""
        return self._records(self.block, slot, count)

    def clear_blocks(self):
        self._call("clear_blocks")


def _bind(L):
    return AcarsBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return AcarsBank.status_array(st)


__all__ = ["AcarsBank", "AcarsConfig", "AcarsParams", "AcarsSlot", "acars_params", "status_array", "Slot", "Record",
           "STATUS_DTYPE", "STATUS_WORDS", "INFO_DTYPE", "MAX_SLOTS", "MAX_BLOCK_BYTES", "GOOD", "ENDED_BY_ETB", "OVERRUN"]
