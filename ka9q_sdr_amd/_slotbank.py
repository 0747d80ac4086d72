"""What the Python mirrors of the PCM decoder banks share (tone.py, cw.py, rtty.py, psk.py, acars.py, ale.py, dsc.py,
navtex.py, same.py, fsk.py, pag.py; include/ka9q_hip.h: kq_tone_*, kq_cw_*, kq_rtty_*, kq_psk_*, kq_acars_*, kq_ale_*,
kq_dsc_*, kq_navtex_*, kq_same_*, kq_fsk_*, kq_pag_*): the ctypes binding of the entry points they all have, and the methods
that differ only in the C prefix.  A module keeps its structures, dtypes and constants, its __init__ and the getters that are its own.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library
from .packet import KQ_PCM_F32, KQ_PCM_S16BE

_P, _U, _Z = C.c_void_p, C.c_uint, C.c_size_t


class SlotBank(Handle):
    """A bank of up to max_slots decoders, each on one source row.  A subclass names the C prefix (`_prefix`, "kq_cw"), its
    config and params structures with the function that makes the params from keywords (`_config`, `_params`,
    `_make_params`), `_status` (STATUS_DTYPE), `_article` for the error text, Handle's `_destroy`, and in `_entry` the
    argument types, behind the handle, of the entry points of its own; its __init__ calls _create() and sets max_slots,
    device and stream."""
    _prefix = _config = _params = _make_params = _status = None
    _article = "a"
    _entry = {}
    _process_more = []      # argument types of kq_*_process behind status and its stride
    _int_rate = False       # the config's samprate is an int

    @classmethod
    def _bind(cls, L):
        p = cls._prefix
        if getattr(L, "_%s_bound" % p, False):
            return L
        entry = {"destroy": [], "set": [_U, C.POINTER(cls._params)], "remove": [_U],
                 "process": [_P, C.c_int, _Z, _Z, _U, _U, C.c_int, _P, _Z] + cls._process_more,
                 "pull_counts": [_P], "sync": [], "reset": []}
        entry.update(cls._entry)
        for name, args in entry.items():
            getattr(L, "%s_%s" % (p, name)).argtypes = [_P] + args
        create = getattr(L, p + "_create")
        create.restype, create.argtypes = _P, [C.POINTER(cls._config)]
        L.kq_bank_stream.restype = _P
        L.kq_bank_stream.argtypes = [_P]
        setattr(L, "_%s_bound" % p, True)
        return L

    def _create(self, *fields):
        """the handle of a bank with the config's fields; no samples taken so far"""
        self.lib = self._bind(load_library())
        self.h = getattr(self.lib, self._prefix + "_create")(C.byref(self._config(*fields)))
        if not self.h:
            raise KqError("%s_create: %s" % (self._prefix, _err(self.lib)))
        self.n = 0

    def _call(self, name, *args):
        what = "%s_%s" % (self._prefix, name)
        return self._chk(getattr(self.lib, what)(self.h, *args), what)

    @classmethod
    def beside(cls, bank, *args, **kw):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D); the
        other arguments as the constructor's, without samprate, max_samples and stream"""
        lib = cls._bind(load_library())
        rate = bank.samprate // bank.D if cls._int_rate else bank.samprate / bank.D
        return cls(rate, *args, max_samples=bank.max_blocks * bank.olen, stream=lib.kq_bank_stream(bank.h), **kw)

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (the module's params structure, or the keywords of its *_params()); it starts cold at
        the next call"""
        p = params if params is not None else type(self)._make_params(**kw)
        self._call("set", slot, C.byref(p))

    def remove(self, slot):
        self._call("remove", slot)

    def _host_input(self, x, nblocks, fmt):
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x, ">i2" if fmt == KQ_PCM_S16BE else np.float32)
        if x.shape[1] % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (x.shape[1], nblocks))
        return x

    def process(self, x, nblocks=1, fmt=KQ_PCM_F32, _more=()):
        """x: host [rows][n] (row = source), float32, or for KQ_PCM_S16BE int16 values that go out in network byte order; n
        split into nblocks equal blocks.  Synchronous.  Returns status: STATUS_DTYPE [max_slots] (empty slots 0)."""
        x = self._host_input(x, nblocks, fmt)
        n = x.shape[1]
        st = np.zeros(self.max_slots, self._status)
        self._call("process", x.ctypes.data, fmt, n, n // nblocks, n // nblocks, nblocks, 0, st.ctypes.data, 1, *_more)
        self.n += n
        return st

    def process_device(self, src_ptr, src_stride, row_stride, block_len, nblocks, status_ptr=None, status_stride=1,
                       fmt=KQ_PCM_F32, _more=()):
        """asynchronous on the handle's stream; every pointer is device memory"""
        self._call("process", src_ptr, fmt, src_stride, row_stride, block_len, nblocks, 1, status_ptr, status_stride, *_more)
        self.n += block_len * nblocks

    def _bank_more(self, torch, **kw):
        """what process_bank hands kq_*_process behind status and its stride"""
        return ()

    def process_bank(self, bank, status=None, **kw):
        """Decode a receiver Bank's last call straight from its device audio plane on the bank's stream, with no host round
        trip and no host wait: kq_bank_join first orders the decode behind the bank's demodulators.  status: a contiguous
        torch device tensor int32 [max_slots][STATUS_WORDS] to write, or None for a new zeroed one (status_array() views
        it as STATUS_DTYPE).  Returns status.  The decode waits for what torch's current stream has queued, and that
        stream waits for the decode."""
        import torch
        name = type(self).__name__
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs %s %s on the bank's stream (%s.beside(bank, ...))" % (self._article, name, name))
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        words = self._status.itemsize // 4
        dev = torch.device("cuda", self.device)
        if status is None:
            status = torch.zeros((self.max_slots, words), dtype=torch.int32, device=dev)
        if not status.is_contiguous() or status.shape != (self.max_slots, words):
            raise ValueError("status must be a contiguous int32 [max_slots][%d]" % words)
        more = self._bank_more(torch, **kw)
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the decoder writes them
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, status.data_ptr(), 1,
                            _more=more)
        cur.wait_stream(ext)
        return status

    def counts(self):
        """records in every slot's arena, uint32 [max_slots]; synchronous"""
        c = np.zeros(self.max_slots, np.uint32)
        self._call("pull_counts", c.ctypes.data)
        return c

    def _records(self, one, slot, count=None):
        """every record of a slot's arena, in order, as one(slot, index) reads them"""
        if count is None:
            count = int(self.counts()[slot])
        return [one(slot, k) for k in range(count)]

    def sync(self):
        self._call("sync")

    def reset(self):
        self._call("reset")
        self.n = 0

    @classmethod
    def status_array(cls, st):
        """a status tensor / int32 array [..][STATUS_WORDS] from process_bank as a STATUS_DTYPE array"""
        a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
        return np.ascontiguousarray(a, np.int32).view(cls._status)[..., 0]


class EventBank(SlotBank):
    """A SlotBank whose arenas hold events: `_event_dtype` (EVENT_DTYPE) and `_event`, the namedtuple of the fields it
    reports."""
    _event_dtype = _event = None
    _entry = {"pull_event": [_U, _U, _P], "clear_events": [], "get_table": [_P, _Z]}

    def get_table(self):
        """C: the cosine table, int16 [1024]"""
        c = np.zeros(1024, np.int16)
        assert self._call("get_table", c.ctypes.data, c.size) == c.size
        return c

    def event(self, slot, index):
        """one event of a slot's arena, an Event; synchronous"""
        r = np.zeros(1, self._event_dtype)
        self._call("pull_event", slot, index, r.ctypes.data)
        return self._event(*(int(r[0][k]) for k in self._event._fields))

    def events(self, slot, count=None):
        """every event of a slot's arena, in order"""
        return self._records(self.event, slot, count)

    def clear_events(self):
        self._call("clear_events")
