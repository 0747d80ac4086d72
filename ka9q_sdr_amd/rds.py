"""Python mirror of the RDS / RBDS decoder bank (include/ka9q_hip.h: kq_rds_*): broadcast FM composites (the discriminator
output of flat FM channels, rad/sample) to RDS groups, up to 4096 slots, and a small host-side reader of those groups
(RdsStation: PI, PTY, TP, programme service name, RadioText).  ctypes over libka9q_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library

MAX_SLOTS = 4096
SUBCARRIER_HZ = 57000.0
BIT_HZ = 1187.5
GROUP_DTYPE = np.dtype([("block", np.uint16, (4,)), ("ok", np.uint8), ("version_b", np.uint8), ("reserved", np.uint16),
                        ("bit", np.uint32)])
STATUS_DTYPE = np.dtype([("phase", np.float32), ("timing", np.float32), ("level", np.float32), ("synced", np.int32),
                         ("blocks_ok", np.uint32), ("blocks_bad", np.uint32)])


class RdsConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("comp_rate", C.c_int), ("decimate", C.c_uint), ("L", C.c_uint), ("M", C.c_uint),
                ("kaiser_beta", C.c_float), ("max_slots", C.c_uint), ("max_samples", C.c_size_t), ("stream", C.c_void_p)]


class RdsParams(C.Structure):
    _fields_ = [("source", C.c_uint), ("track_ms", C.c_float), ("lose_after", C.c_int)]


def rds_params(source=0, track_ms=20.0, lose_after=10):
    """kq_rds_params with the defaults: a 20 ms tracker, sync dropped after 10 bad blocks in a row"""
    return RdsParams(source, track_ms, lose_after)


def _bind(L):
    if getattr(L, "_kq_rds_bound", False):
        return L
    L.kq_rds_create.restype = C.c_void_p
    L.kq_rds_create.argtypes = [C.POINTER(RdsConfig)]
    L.kq_rds_destroy.argtypes = [C.c_void_p]
    L.kq_rds_set.argtypes = [C.c_void_p, C.c_uint, C.POINTER(RdsParams)]
    L.kq_rds_remove.argtypes = [C.c_void_p, C.c_uint]
    L.kq_rds_max_groups.restype = C.c_size_t
    L.kq_rds_max_groups.argtypes = [C.c_void_p, C.c_size_t]
    L.kq_rds_process.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
    L.kq_rds_pull_baseband.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t]
    L.kq_rds_sync.argtypes = [C.c_void_p]
    L.kq_rds_reset.argtypes = [C.c_void_p]
    L.kq_bank_stream.restype = C.c_void_p
    L.kq_bank_stream.argtypes = [C.c_void_p]
    L._kq_rds_bound = True
    return L


class RdsBank(Handle):
    """Up to max_slots RDS decoders on one composite geometry (Fc = comp_rate, Dr = decimate, frames of L, filter of M).
    For process_bank, create it on the receiver bank's stream: RdsBank.beside(bank, ...)."""
    _destroy = "kq_rds_destroy"

    def __init__(self, comp_rate, decimate, L, M, max_slots, max_samples, kaiser_beta=3.0, device=0, stream=None):
        self.lib = _bind(load_library())
        cfg = RdsConfig(device, comp_rate, decimate, L, M, kaiser_beta, max_slots, max_samples, stream)
        self.h = self.lib.kq_rds_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_rds_create: " + _err(self.lib))
        self.comp_rate, self.decimate, self.L, self.M = comp_rate, decimate, L, M
        self.max_slots, self.max_samples, self.device, self.stream = max_slots, max_samples, device, stream
        self.Lr = L // decimate
        self.n = 0   # composite samples taken so far

    @classmethod
    def beside(cls, bank, decimate, L, M, max_slots, kaiser_beta=3.0):
        """a decoder bank on a receiver Bank's stream, sized for its calls, decoding its output rate (samprate / D)"""
        lib = _bind(load_library())
        rate = bank.samprate // bank.D
        return cls(rate, decimate, L, M, max_slots, bank.max_blocks * bank.olen, kaiser_beta,
                   stream=lib.kq_bank_stream(bank.h))

    def set(self, slot, params=None, **kw):
        """put a decoder in `slot` (an RdsParams, or rds_params() keywords); it starts cold at the next call"""
        p = params if params is not None else rds_params(**kw)
        self._chk(self.lib.kq_rds_set(self.h, slot, C.byref(p)), "kq_rds_set")

    def remove(self, slot):
        self._chk(self.lib.kq_rds_remove(self.h, slot), "kq_rds_remove")

    def frames(self, nsamples):
        """frames the next call of nsamples completes"""
        return (self.n + nsamples) // self.L - self.n // self.L

    def max_groups(self, nsamples):
        """the bound on groups per slot of a call of nsamples"""
        return int(self.lib.kq_rds_max_groups(self.h, nsamples))

    def process(self, comp, nblocks=1):
        """comp: host float32 [rows][n] (row = source), n split into nblocks equal blocks.  Synchronous.  Returns
        (groups GROUP_DTYPE [max_slots][max_groups(n)], counts uint32 [max_slots], status STATUS_DTYPE [max_slots][F]);
        groups[s, :counts[s]] are slot s's; rows of empty slots are 0."""
        comp = np.ascontiguousarray(comp, np.float32)
        if comp.ndim == 1:
            comp = comp[None, :]
        n = comp.shape[1]
        if n % nblocks:
            raise ValueError("%d samples do not split into %d blocks" % (n, nblocks))
        F = self.frames(n)
        cap = self.max_groups(n)
        groups = np.zeros((self.max_slots, cap), GROUP_DTYPE)
        counts = np.zeros(self.max_slots, np.uint32)
        st = np.zeros((self.max_slots, F), STATUS_DTYPE)
        got = self._chk(self.lib.kq_rds_process(self.h, comp.ctypes.data, n, n // nblocks, n // nblocks, nblocks, 0,
                                                groups.ctypes.data, cap, counts.ctypes.data, st.ctypes.data, F),
                        "kq_rds_process")
        assert got == F
        self.n += n
        return groups, counts, st

    def process_device(self, comp_ptr, src_stride, row_stride, block_len, nblocks, groups_ptr=None, groups_stride=0,
                       counts_ptr=None, status_ptr=None, status_stride=0):
        """asynchronous on the handle's stream; every pointer is device memory.  Returns F."""
        F = self._chk(self.lib.kq_rds_process(self.h, comp_ptr, src_stride, row_stride, block_len, nblocks, 1, groups_ptr,
                                              groups_stride, counts_ptr, status_ptr, status_stride), "kq_rds_process")
        self.n += block_len * nblocks
        return F

    def process_bank(self, bank, groups=None, counts=None, status=None):
        """Decode a receiver Bank's last call straight from its device audio plane (flat FM channels: the composite) on the
        bank's stream, with no host round trip and no host wait: kq_bank_join first orders the decode behind the bank's
        demodulators, wherever the bank ran them.  groups / counts / status: contiguous torch device tensors int32
        [max_slots][>= max_groups][4], int32 [max_slots] and int32 [max_slots][>= F][6] to write, or None for new zeroed
        ones.  Returns (F, groups, counts, status[:, :F]); group_array() / status_array() view them as GROUP_DTYPE /
        STATUS_DTYPE.  The decode waits for what torch's current stream has queued, and that stream waits for the decode,
        so the tensors are used there as any others."""
        import torch
        if self.stream is None or self.stream != self.lib.kq_bank_stream(bank.h):
            raise ValueError("process_bank needs an RdsBank on the bank's stream (RdsBank.beside(bank, ...))")
        nb = bank.lib.kq_bank_last_blocks(bank.h)
        olen = bank.olen
        F = self.frames(nb * olen)
        cap = self.max_groups(nb * olen)
        dev = torch.device("cuda", self.device)
        if groups is None:
            groups = torch.zeros((self.max_slots, cap, 4), dtype=torch.int32, device=dev)
        if counts is None:
            counts = torch.zeros((self.max_slots,), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.zeros((self.max_slots, max(F, 1), 6), dtype=torch.int32, device=dev)
        if not (groups.is_contiguous() and counts.is_contiguous() and status.is_contiguous()) or groups.shape[1] < cap \
                or status.shape[1] < F:
            raise ValueError("groups / counts / status must be contiguous and hold %d groups / %d frames per slot" % (cap, F))
        ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext.wait_stream(cur)   # the buffers, made or last used on torch's stream, before the decoder writes them
        bank.join()            # the demodulators that write the plane, before the decoder reads it
        got = self.process_device(bank.audio_device_ptr(), bank.max_blocks * 2 * olen, 2 * olen, olen, nb, groups.data_ptr(),
                                  groups.shape[1], counts.data_ptr(), status.data_ptr(), status.shape[1])
        assert got == F
        # torch's stream waits for the decode, so a later use or reuse of the buffers there comes after it.  (No
        # record_stream on the bank's stream: see WfmBank.process_bank.)
        cur.wait_stream(ext)
        return F, groups, counts, status[:, :F]

    def pull_baseband(self, slot):
        """the last call's z of a slot, complex64 [F Lr]; synchronous"""
        cap = (self.max_samples // self.L + 1) * self.Lr
        buf = np.zeros(cap, np.complex64)
        got = self._chk(self.lib.kq_rds_pull_baseband(self.h, slot, buf.ctypes.data, cap), "kq_rds_pull_baseband")
        return buf[:got]

    def sync(self):
        self._chk(self.lib.kq_rds_sync(self.h), "kq_rds_sync")

    def reset(self):
        self._chk(self.lib.kq_rds_reset(self.h), "kq_rds_reset")
        self.n = 0


def group_array(g):
    """a groups tensor / int32 array [..][4] from process_bank as a GROUP_DTYPE array"""
    a = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
    return np.ascontiguousarray(a, np.int32).view(GROUP_DTYPE)[..., 0]


def status_array(st):
    """a status tensor / int32 array [..][6] from process_bank as a STATUS_DTYPE array"""
    a = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    return np.ascontiguousarray(a, np.int32).view(STATUS_DTYPE)[..., 0]


def _char(c):
    return chr(c) if 0x20 <= c < 0x7F else "?"


class RdsStation:
    """A reader of one station's group records (GROUP_DTYPE elements, or (block[4], ok, version_b) tuples): PI, PTY and TP
    from blocks A and B, the 8-character programme service name from groups 0A / 0B, RadioText from 2A / 2B.  Only blocks
    whose ok bit is set are used; characters outside printable ASCII show as '?', places not yet received as ' '."""

    def __init__(self):
        self.pi = self.pty = self.tp = None
        self._ps = [None] * 8
        self._rt = [None] * 64
        self._rt_flag = None
        self.groups = 0

    @property
    def ps(self):
        return "".join(" " if c is None else _char(c) for c in self._ps)

    @property
    def ps_complete(self):
        return all(c is not None for c in self._ps)

    @property
    def radiotext(self):
        out = []
        for c in self._rt:
            if c == 0x0D:    # end of text
                break
            out.append(" " if c is None else _char(c))
        return "".join(out).rstrip()

    def feed(self, records):
        """take group records in order; returns self"""
        if isinstance(records, np.ndarray) and records.dtype == GROUP_DTYPE:
            records = [(r["block"], r["ok"], r["version_b"]) for r in records.reshape(-1)]
        for rec in records:
            self._group([int(v) for v in rec[0]], int(rec[1]))
        return self

    def _group(self, blk, ok):
        self.groups += 1
        if ok & 1:
            self.pi = blk[0]
        if not ok & 2:
            return                      # without block B nothing else can be placed
        b = blk[1]
        gtype, ver_b = b >> 12, (b >> 11) & 1
        self.tp, self.pty = (b >> 10) & 1, (b >> 5) & 31
        if ver_b and ok & 4:
            self.pi = blk[2]            # version B repeats PI in block C'
        if gtype == 0 and ok & 8:
            a = b & 3
            self._ps[2 * a], self._ps[2 * a + 1] = blk[3] >> 8, blk[3] & 0xFF
        elif gtype == 2:
            flag, a = (b >> 4) & 1, b & 15
            if self._rt_flag is not None and flag != self._rt_flag:
                self._rt = [None] * 64  # the A/B flag toggled: a new text
            self._rt_flag = flag
            if ver_b:
                if ok & 8:
                    self._rt[2 * a], self._rt[2 * a + 1] = blk[3] >> 8, blk[3] & 0xFF
            else:
                if ok & 4:
                    self._rt[4 * a], self._rt[4 * a + 1] = blk[2] >> 8, blk[2] & 0xFF
                if ok & 8:
                    self._rt[4 * a + 2], self._rt[4 * a + 3] = blk[3] >> 8, blk[3] & 0xFF


__all__ = ["RdsBank", "RdsConfig", "RdsParams", "RdsStation", "rds_params", "group_array", "status_array", "GROUP_DTYPE",
           "STATUS_DTYPE", "MAX_SLOTS"]
