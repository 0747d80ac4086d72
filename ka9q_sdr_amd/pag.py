"""Python mirror of the POCSAG pager decoder bank (include/ka9q_hip.h: kq_pag_*): the discriminator output of flat FM
channels (rad/sample) to pages at 512, 1200 or 2400 bit/s, up to 4096 slots.  ctypes over libka9q_hip.so; there is no CPU
path.  pocsag.py reads the pages (numeric, alpha) and makes test traffic (encode).
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library
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


def _bind(L):
    if getattr(L, "_kq_pag_bound", False):
        return L
    L.kq_pag_create.restype = C.c_void_p
    L.kq_pag_create.argtypes = [C.POINTER(PagConfig)]
    L.kq_pag_destroy.argtypes = [C.c_void_p]
    L.kq_pag_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(PagParams)]
    L.kq_pag_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_pag_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int,
                                 C.c_void_p, C.c_size_t]
    L.kq_pag_pull_counts.argtypes = [C.c_void_p, C.c_void_p]
    L.kq_pag_pull_page.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p]
    L.kq_pag_clear_pages.argtypes = [C.c_void_p]
    L.kq_pag_get_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_pag_sync.argtypes = [C.c_void_p]
    L.kq_pag_reset.argtypes = [C.c_void_p]
    L.kq_pag_correct.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_pag_bound = True
    return L


def correct(word):
    """(codeword, bits changed: 0, 1 or 2) of a received 32-bit word, or (None, -1): kq_pag_correct, host only"""
    lib = _bind(load_library())
    out = C.c_uint32(0)
    n = lib.kq_pag_correct(word & 0xFFFFFFFF, C.byref(out))
    return (out.value, n) if n >= 0 else (None, -1)


class PagBank(Handle):
    """Up to max_slots decoders on one geometry (Fs = samprate, baud, a low-pass of `taps`, a threshold window of
    window_bits bits).  For process_bank, create it on the receiver bank's stream: PagBank.beside(bank, ...)."""
    _destroy = "kq_pag_destroy"

    def __init__(self, samprate, baud, taps, max_slots, max_samples, cutoff_hz=None, kaiser_beta=2.0, window_bits=None,
                 input_scale=4096.0, pll_shift=3, max_pages=16, max_page_words=64, device=0, stream=None):
        self.lib = _bind(load_library())
        if cutoff_hz is None:
            cutoff_hz = 0.75 * baud
        if window_bits is None:
            window_bits = default_window_bits(samprate, baud)
        cfg = PagConfig(device, samprate, baud, taps, cutoff_hz, kaiser_beta, window_bits, input_scale, pll_shift, max_slots,
                        max_pages, max_page_words, max_samples, stream)
        self.h = self.lib.kq_pag_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_pag_create: " + _err(self.lib))
        self.samprate, self.baud, self.taps = samprate, baud, taps
        self.cutoff_hz, self.kaiser_beta, self.window_bits = cutoff_hz, kaiser_beta, window_bits
        self.max_slots, self.max_samples, self.max_pages, self.max_page_words = max_slots, max_samples, max_pages, max_page_words
        self.device, self.stream = device, stream
        self.n = 0   # samples taken so far

    @classmethod
    def beside(cls, bank, baud, taps, max_slots, **kw):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D)"""
        lib = _bind(load_library())
        return cls(bank.samprate / bank.D, baud, taps, max_slots, bank.max_blocks * bank.olen,
                   stream=lib.kq_bank_stream(bank.h), **kw)

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (a PagParams, or pag_params() keywords); it starts cold at the next call"""
        p = params if params is not None else pag_params(**kw)
        self._chk(self.lib.kq_pag_set(self.h, slot, C.byref(p)), "kq_pag_set")

    def remove(self, slot):
        self._chk(self.lib.kq_pag_remove(self.h, slot), "kq_pag_remove")

    def get_taps(self):
        """hq: the quantised low-pass, int16 [taps]"""
        hq = np.zeros(self.taps, np.int16)
        assert self._chk(self.lib.kq_pag_get_taps(self.h, hq.ctypes.data, self.taps), "kq_pag_get_taps") == self.taps
        return hq

    def process(self, x, nblocks=1, fmt=KQ_PCM_F32):
        """x: host [rows][n] (row = source), float32, or for KQ_PCM_S16BE int16 values that go out in network byte order; n
        split into nblocks equal blocks.  Synchronous.  Returns status, STATUS_DTYPE [max_slots] (rows of empty slots 0)."""
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x, ">i2" if fmt == KQ_PCM_S16BE else np.float32)
        n = x.shape[1]
        if n % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (n, nblocks))
        st = np.zeros(self.max_slots, STATUS_DTYPE)
        self._chk(self.lib.kq_pag_process(self.h, x.ctypes.data, fmt, n, n // nblocks, n // nblocks, nblocks, 0, st.ctypes.data,
                                          1), "kq_pag_process")
        self.n += n
        return st

    def process_device(self, src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr=None, status_stride=1,
                       fmt=KQ_PCM_F32):
        """asynchronous on the handle's stream; every pointer is device memory"""
        self._chk(self.lib.kq_pag_process(self.h, src_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, status_ptr,
                                          status_stride), "kq_pag_process")
        self.n += block_len * nblocks

    def process_bank(self, bank, status=None):
        """Decode a receiver Bank's last call straight from its device audio plane (flat FM channels) on the bank's stream,
        with no host round trip and no host wait: kq_bank_join first orders the decode behind the bank's demodulators.
        status: a contiguous torch device tensor int32 [max_slots][STATUS_WORDS] to write, or None for a new zeroed one
        (status_array() views it as STATUS_DTYPE).  Returns it.  The decode waits for what torch's current stream has
        queued, and that stream waits for the decode."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs a PagBank on the bank's stream (PagBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        dev = torch.device("cuda", self.device)
        if status is None:
            status = torch.zeros((self.max_slots, STATUS_WORDS), dtype=torch.int32, device=dev)
        if not status.is_contiguous() or status.shape != (self.max_slots, STATUS_WORDS):
            raise ValueError("status must be a contiguous int32 [max_slots][%d]" % STATUS_WORDS)
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffer, made or last used on torch's stream, before the decoder writes it
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, status.data_ptr(), 1)
        cur.wait_stream(ext)
        return status

    def counts(self):
        """pages in every slot's arena, uint32 [max_slots]; synchronous"""
        c = np.zeros(self.max_slots, np.uint32)
        self._chk(self.lib.kq_pag_pull_counts(self.h, c.ctypes.data), "kq_pag_pull_counts")
        return c

    def page(self, slot, index):
        """one page of a slot's arena, a pocsag.Page (ric, function, words, flags, errors, end_sample); synchronous"""
        buf = np.zeros(3 * self.max_page_words, np.uint8)
        info = np.zeros(1, INFO_DTYPE)
        n = self._chk(self.lib.kq_pag_pull_page(self.h, slot, index, buf.ctypes.data, buf.size, info.ctypes.data),
                      "kq_pag_pull_page")
        r = info[0]
        assert n == 3 * int(r["nwords"])
        return Page(int(r["ric"]), int(r["function"]), bytes(buf[:n]), int(r["flags"]), int(r["errors"]), int(r["end_sample"]))

    def pages(self, slot, count=None):
        """every page of a slot's arena, in order"""
        if count is None:
            count = int(self.counts()[slot])
        return [self.page(slot, k) for k in range(count)]

    def clear_pages(self):
        self._chk(self.lib.kq_pag_clear_pages(self.h), "kq_pag_clear_pages")

    def sync(self):
        self._chk(self.lib.kq_pag_sync(self.h), "kq_pag_sync")

    def reset(self):
        self._chk(self.lib.kq_pag_reset(self.h), "kq_pag_reset")
        self.n = 0


def status_array(st):
    """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


__all__ = ["PagBank", "PagConfig", "PagParams", "pag_params", "correct", "default_window_bits", "status_array", "STATUS_DTYPE",
           "STATUS_WORDS", "INFO_DTYPE", "MAX_SLOTS", "TILE"]
