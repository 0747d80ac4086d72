"""Python mirror of the POCSAG pager decoder bank (include/ka9q_hip.h: kq_pag_*): the discriminator output of flat FM
channels (rad/sample) to pages at 512, 1200 or 2400 bit/s, up to 4096 slots.  ctypes over libka9q_hip.so; there is no CPU
path.  pocsag.py reads the pages (numeric, alpha) and makes test traffic (encode).
"""
import ctypes as C

import numpy as np

from ._slotbank import SlotBank
from .bank import load_library
from .packet import KQ_PCM_F32, KQ_PCM_S16BE
from .pocsag import Page

MAX_SLOTS = 4096
TILE = 1024          # samples per workgroup of k_fsk_front (a seam for call splits)
STATUS_DTYPE = np.dtype([("bits", np.uint32), ("syncs", np.uint32), ("batches", np.uint32), ("sync_missed", np.uint32),
                         ("words_good", np.uint32), ("words_fixed", np.uint32), ("words_bad", np.uint32), ("orphans", np.uint32),
                         ("pages", np.uint32), ("dropped", np.uint32), ("pll_phase", np.int32), ("synced", np.int32),
                         ("inverted", np.int32), ("level", np.uint32)])
STATUS_WORDS = STATUS_DTYPE.itemsize // 4
INFO_DTYPE = np.dtype([("ric", np.uint32), ("function", np.uint32), ("nwords", np.uint32), ("flags", np.uint32),
                       ("errors", np.uint32), ("reserved", np.uint32), ("end_sample", np.uint64)])


class PagConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_double), ("baud", C.c_int), ("taps", C.c_uint), ("cutoff_hz", C.c_float),
                ("kaiser_beta", C.c_float), ("window_bits", C.c_float), ("input_scale", C.c_float), ("pll_shift", C.c_int),
                ("max_slots", C.c_uint), ("max_pages", C.c_uint), ("max_page_words", C.c_uint), ("max_samples", C.c_size_t),
                ("stream", C.c_void_p)]


class PagParams(C.Structure):
    _fields_ = [("source", C.c_uint)]


def pag_params(source=0):
    """kq_pag_params"""
    return PagParams(source)


def default_window_bits(samprate, baud):
    """the widest threshold window the limits allow, 24 bits at most: min(24, 1024 baud / Fs - 0.5)"""
    return min(24.0, 1024.0 * baud / samprate - 0.5)


def correct(word):
    """(codeword, bits changed: 0, 1 or 2) of a received 32-bit word, or (None, -1): kq_pag_correct, host only"""
    lib = _bind(load_library())
    out = C.c_uint32(0)
    n = lib.kq_pag_correct(word & 0xFFFFFFFF, C.byref(out))
    return (out.value, n) if n >= 0 else (None, -1)


class PagBank(SlotBank):
    """Up to max_slots decoders on one geometry (Fs = samprate, baud, a low-pass of `taps`, a threshold window of
    window_bits bits), on the discriminator output of flat FM channels.  For process_bank, create it on the receiver
    bank's stream: PagBank.beside(bank, ...)."""
    _destroy = "kq_pag_destroy"
    _prefix, _config, _params, _make_params, _status = "kq_pag", PagConfig, PagParams, staticmethod(pag_params), STATUS_DTYPE
    _entry = {"pull_page": [C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p], "clear_pages": [],
              "get_taps": [C.c_void_p, C.c_size_t]}

    def __init__(self, samprate, baud, taps, max_slots, max_samples, cutoff_hz=None, kaiser_beta=2.0, window_bits=None,
                 input_scale=4096.0, pll_shift=3, max_pages=16, max_page_words=64, device=0, stream=None):
        if cutoff_hz is None:
            cutoff_hz = 0.75 * baud
        if window_bits is None:
            window_bits = default_window_bits(samprate, baud)
        self._create(device, samprate, baud, taps, cutoff_hz, kaiser_beta, window_bits, input_scale, pll_shift, max_slots,
                     max_pages, max_page_words, max_samples, stream)
        self.samprate, self.baud, self.taps = samprate, baud, taps
        self.cutoff_hz, self.kaiser_beta, self.window_bits = cutoff_hz, kaiser_beta, window_bits
        self.max_slots, self.max_samples, self.max_pages, self.max_page_words = max_slots, max_samples, max_pages, max_page_words
        self.device, self.stream = device, stream

    def get_taps(self):
        """hq: the quantised low-pass, int16 [taps]"""
        hq = np.zeros(self.taps, np.int16)
        assert self._call("get_taps", hq.ctypes.data, self.taps) == self.taps
        return hq

    def page(self, slot, index):
        """one page of a slot's arena, a pocsag.Page (ric, function, words, flags, errors, end_sample); synchronous"""
        buf = np.zeros(3 * self.max_page_words, np.uint8)
        info = np.zeros(1, INFO_DTYPE)
        n = self._call("pull_page", slot, index, buf.ctypes.data, buf.size, info.ctypes.data)
        r = info[0]
        assert n == 3 * int(r["nwords"])
        return Page(int(r["ric"]), int(r["function"]), bytes(buf[:n]), int(r["flags"]), int(r["errors"]), int(r["end_sample"]))

    def pages(self, slot, count=None):
        """every page of a slot's arena, in order"""
        return self._records(self.page, slot, count)

    def clear_pages(self):
        self._call("clear_pages")


def _bind(L):
    L.kq_pag_correct.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
    return PagBank._bind(L)


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    return PagBank.status_array(st)


__all__ = ["PagBank", "PagConfig", "PagParams", "pag_params", "correct", "default_window_bits", "status_array", "STATUS_DTYPE",
           "STATUS_WORDS", "INFO_DTYPE", "MAX_SLOTS", "TILE"]
