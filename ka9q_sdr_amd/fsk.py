"""Python mirror of the baseband FSK / GMSK packet decoder bank (include/ka9q_hip.h: kq_fsk_*): the discriminator output of
flat FM channels (rad/sample) to HDLC frames, 9600 bit/s G3RUH packet and AIS, up to 4096 slots.  ctypes over
libka9q_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from ._slotbank import SlotBank
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

MAX_SLOTS = 4096
TILE = 1024          # samples per workgroup of k_fsk_front (a seam for call splits)
STATUS_DTYPE = np.dtype([("bits", np.uint32), ("frames_good", np.uint32), ("frames_bad", np.uint32), ("aborts", np.uint32),
                         ("dropped", np.uint32), ("pll_phase", np.int32), ("in_frame", np.int32), ("level", np.uint32)])
INFO_DTYPE = np.dtype([("length", np.uint32), ("end_bit", np.uint32), ("end_sample", np.uint64)])


class FskConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_int), ("baud", C.c_int), ("taps", C.c_uint), ("cutoff_hz", C.c_float),
                ("kaiser_beta", C.c_float), ("window_bits", C.c_float), ("input_scale", C.c_float), ("pll_shift", C.c_int),
                ("max_slots", C.c_uint), ("max_frames", C.c_uint), ("max_frame_bytes", C.c_uint), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class FskParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("scrambled", C.c_int), ("min_bytes", C.c_uint)]


def fsk_params(source=0, scrambled=1, min_bytes=8):
    """kq_fsk_params with the defaults: G3RUH (scrambled=0: AIS), candidates of 8 bytes and more"""
    return FskParams(source, int(scrambled), min_bytes)


class FskBank(SlotBank):
    """Up to max_slots decoders on one geometry (Fs = samprate, baud, a low-pass of `taps`, a threshold window of
    window_bits bits), on the discriminator output of flat FM channels.  For process_bank, create it on the receiver
    bank's stream: FskBank.beside(bank, ...)."""
    _destroy = "kq_fsk_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_fsk", FskConfig, FskParams, staticmethod(fsk_params), STATUS_DTYPE
    _article, _int_rate = "an", True
    _entry = {"pull_frame": [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p], "clear_frames": [],
              "get_taps": [C.c_void_p, C.c_size_t]}

    def __init__(self, samprate, baud, taps, max_slots, max_samples, cutoff_hz=None, kaiser_beta=2.0, window_bits=16.0,
                 input_scale=4096.0, pll_shift=3, max_frames=16, max_frame_bytes=512, device=0, stream=None):
        if cutoff_hz is None:
            cutoff_hz = 0.6 * baud
        self._create(device, samprate, baud, taps, cutoff_hz, kaiser_beta, window_bits, input_scale, pll_shift, max_slots,
                     max_frames, max_frame_bytes, max_samples, stream)
        self.samprate, self.baud, self.taps = samprate, baud, taps
        self.max_slots, self.max_samples, self.max_frame_bytes = max_slots, max_samples, max_frame_bytes
        self.device, self.stream = device, stream

    def get_taps(self):
        """hq: the quantised low-pass, int16 [taps]"""
        hq = np.zeros(self.taps, np.int16)
        assert self._call("get_taps", hq.ctypes.data, self.taps) == self.taps
        return hq

    def frame(self, slot, index):
        """(bytes, end_sample, end_bit) of one frame of a slot's arena; synchronous"""
        buf = np.zeros(self.max_frame_bytes, np.uint8)
        info = np.zeros(1, INFO_DTYPE)
        n = self._call("pull_frame", slot, index, buf.ctypes.data, buf.size, info.ctypes.data)
        assert n == int(info[0]["length"])
        return bytes(buf[:n]), int(info[0]["end_sample"]), int(info[0]["end_bit"])

    def frames(self, slot, count=None):
        """every frame of a slot's arena, in order, as (bytes, end_sample, end_bit)"""
        return self._records(self.frame, slot, count)

    def clear_frames(self):
        self._call("clear_frames")


def _bind(L):
    return FskBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][8] from process_bank as a STATUS_DTYPE array"""
    return FskBank.status_array(st)


__all__ = ["FskBank", "FskConfig", "FskParams", "fsk_params", "status_array", "STATUS_DTYPE", "INFO_DTYPE", "MAX_SLOTS", "TILE"]
