"""The argument checks that every PCM decoder bank's C interface answers alike (kq_tone, kq_cw, kq_rtty, kq_psk, kq_acars,
kq_ale, kq_dsc, kq_fsk, kq_pag), written once: tests/test_<bank>_args.py describes its bank to Suite -- the prefix, the
ctypes structures, the default config, the dtypes and its tables of bad values, as literal data -- and takes the fixtures
and the shared tests from it under the names they always had.  None of them needs a device.

pytest does not rewrite the asserts of a helper module, so every assert here carries what it compared."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq


class Suite:
    """prefix: "rtty" for kq_rtty_*.  config, params, bind: the ctypes config structure, the params maker and the binder of
    ka9q_sdr_amd/<bank>.py.  default: the config the tests start from, field by field in the structure's order, with
    max_slots 8 and max_samples 2^14 (cfg: a maker of the bank's own in its place).  status: the status dtype.
    record: what the arena holds ("event": kq_*_pull_event, kq_*_clear_events, "slot 0 has 0 events").
    pull: a good pull's arguments behind (bank, slot, index), the destination first; null_pull: what a null one is called.
    slot_limit: the limit on max_slots.  bad_configs: (fields, reason) pairs for kq_*_create.  bad_params: (fields, reason)
    pairs for kq_*_set.  more_slot_checks(lib, bank): the bank's own part of the slot test, behind bad_params.
    null_handles: (entry point, arguments behind the handle) pairs.  set_needs_device: kq_*_set asks for the device (so a
    slot cannot be set and removed here).  process_extra: the arguments of kq_*_process behind status_stride when unused;
    bad_process: (those arguments, reason) pairs.  first_call: see _first_call()."""

    def __init__(self, prefix, config, params, bind, status, record, pull, null_pull, bad_configs, null_handles, default=None,
                 cfg=None, slot_limit=16384, bad_params=(), more_slot_checks=None, set_needs_device=False, process_extra=(),
                 bad_process=(), first_call=None):
        self.prefix, self.params, self.status, self.record, self.slot_limit = prefix, params, status, record, slot_limit
        self.pull_args, self.null_pull = tuple(pull), null_pull
        self.bad_params, self.more_slot_checks = bad_params, more_slot_checks
        self.handles, self.set_needs_device, self.first = null_handles, set_needs_device, first_call
        self.extra, self.more_process = tuple(process_extra), bad_process
        self.cfg = cfg or (lambda **kw: config(*dict(default, **kw).values()))

        @pytest.fixture(scope="module", name="lib")
        def lib():
            kq.build_library()
            return bind(kq.load_library())

        @pytest.fixture(name="bank")
        def bank(lib):
            h = self.fn(lib, "create")(C.byref(self.cfg()))
            assert h, lib.kq_last_error()
            yield h
            assert self.fn(lib, "destroy")(h) == 0, lib.kq_last_error()

        self.lib, self.bank = lib, bank
        self.bad_config = pytest.mark.parametrize("kw,why", bad_configs)(self._bad_config())
        # the tests, as plain functions of their fixtures (pytest does not read a bound method's signature)
        self.null_config, self.null_handles, self.first_call = (
            lambda lib, f=f: f(lib) for f in (self._null_config, self._null_handles, self._first_call))
        self.bad_slot, self.bad_process, self.without_a_slot = (
            lambda lib, bank, f=f: f(lib, bank) for f in (self._bad_slot, self._bad_process, self._without_a_slot))

    def name(self, entry):
        return ("kq_%s_%s" % (self.prefix, entry)).encode()

    def fn(self, lib, entry):
        return getattr(lib, self.name(entry).decode())

    def refused(self, lib, got, why, *what, whole=False):
        """the call gave -1 and the reason holds `why` (whole: is `why` behind the entry point's name)"""
        msg = lib.kq_last_error()
        assert got == -1, (got, msg) + what
        assert (msg == why) if whole else (why in msg), (msg, why) + what

    def _null_config(self, lib):
        got, msg = self.fn(lib, "create")(None), lib.kq_last_error()
        assert got is None and msg == self.name("create") + b": null config", (got, msg)

    def _bad_config(self):
        def test(lib, kw, why):
            got, msg = self.fn(lib, "create")(C.byref(self.cfg(**kw))), lib.kq_last_error()
            assert got is None and msg.startswith(self.name("create") + b": ") and why in msg, (kw, why, got, msg)
        return test

    def _bad_slot(self, lib, bank):
        """the slot against the limits, the null arguments of set, remove, the pull and the counts; max_slots = 8"""
        p, set_, remove, pull = self.params(), self.fn(lib, "set"), self.fn(lib, "remove"), self.fn(lib, "pull_" + self.record)
        self.refused(lib, set_(None, self.slot_limit, C.byref(p)), b"slot %d" % self.slot_limit)
        self.refused(lib, set_(bank, 8, C.byref(p)), b"slot 8 >= max_slots 8")
        self.refused(lib, set_(bank, 0, None), self.name("set") + b": null params", whole=True)
        self.refused(lib, set_(None, 0, C.byref(p)), self.name("set") + b": null bank", whole=True)
        for kw, why in self.bad_params:
            got, msg = set_(bank, 0, C.byref(self.params(**kw))), lib.kq_last_error()
            assert got == -1 and msg.startswith(self.name("set") + b": ") and why in msg, (kw, why, got, msg)
        if self.more_slot_checks:
            self.more_slot_checks(lib, bank)
        self.refused(lib, remove(bank, 3), b"slot 3 holds no decoder")
        self.refused(lib, remove(bank, 8), b"slot 8")
        self.refused(lib, pull(bank, 9, 0, *self.pull_args), b"slot 9 >= max_slots 8")
        self.refused(lib, pull(bank, 0, 0, None, *self.pull_args[1:]), self.name("pull_" + self.record) + b": " + self.null_pull,
                     whole=True)
        self.refused(lib, self.fn(lib, "pull_counts")(bank, None), self.name("pull_counts") + b": null counts", whole=True)

    def _bad_process(self, lib, bank):
        buf, st, x, process = np.zeros(1 << 15, np.float32), np.zeros(8, self.status), self.extra, self.fn(lib, "process")
        src = buf.ctypes.data
        for args, why in [((src, 0, 0, 4096, 4096, 5, 0, None, 0) + x, b"max_samples"),                # 20480 > 16384
                          ((src, 0, 0, 100, 200, 2, 0, None, 0) + x, b"row_stride 100 < block_len 200"),
                          ((src, 2, 0, 16, 16, 1, 0, None, 0) + x, b"unknown sample format 2"),        # KQ_PCM_S16: the modulator's
                          ((src, 0, 0, 16, 16, 1, 0, st.ctypes.data, 0) + x, b"status_stride 0 < 1")] + \
                         [((src, 0, 0, 16, 16, 1, 0, None, 0) + tuple(more), why) for more, why in self.more_process] + \
                         [((None, 0, 0, 16, 16, 1, 0, None, 0) + x, b"null src")]:
            self.refused(lib, process(bank, *args), why, args)
        got = process(bank, None, 0, 0, 0, 0, 0, 0, None, 0, *x)                                         # nothing to do
        assert got == 0, (got, lib.kq_last_error())
        self.refused(lib, process(None, src, 0, 0, 16, 16, 1, 0, None, 0, *x), self.name("process") + b": null bank", whole=True)

    def _without_a_slot(self, lib, bank):
        """with no slot set -- or, where set asks for no device, one set and removed again -- process, counts, clear, sync
        and reset succeed and touch no device"""
        buf = np.zeros(1 << 14, np.float32)
        if not self.set_needs_device:
            got = self.fn(lib, "set")(bank, 5, C.byref(self.params())), self.fn(lib, "remove")(bank, 5)
            assert got == (0, 0), (got, lib.kq_last_error())
        for n in (1, 1000, 16384):
            got = self.fn(lib, "process")(bank, buf.ctypes.data, 0, 0, n, n, 1, 0, None, 0, *self.extra)
            assert got == 0, (n, got, lib.kq_last_error())
        counts = np.full(8, 7, np.uint32)
        got = self.fn(lib, "pull_counts")(bank, counts.ctypes.data)
        assert got == 0 and not counts.any(), (got, counts, lib.kq_last_error())
        for entry in ("clear_%ss" % self.record, "sync", "reset"):
            got = self.fn(lib, entry)(bank)
            assert got == 0, (entry, got, lib.kq_last_error())
        got = self.fn(lib, "pull_" + self.record)(bank, 0, 0, *self.pull_args)
        self.refused(lib, got, b"slot 0 has 0 %ss" % self.record.encode())

    def _null_handles(self, lib):
        for entry, args in self.handles:
            self.refused(lib, self.fn(lib, entry)(None, *args), b"null bank", entry)

    def _first_call(self, lib):
        """first_call: dict(bank: the Python class; geometry: its leading arguments; set: a slot's fields; read(bank), want:
        what the bank hands out of them; again (optional): the fields the slot is set to once removed; refused: (geometry,
        further arguments, reason) of banks that are not made).  set needs no device, and the first call says where there
        is none"""
        f = self.first
        make = lambda geometry, **kw: f["bank"](*geometry, max_slots=4, max_samples=4096, **kw)
        b = make(f["geometry"])
        b.set(0, **f["set"])                                             # no device asked for yet
        got = f["read"](b)
        assert got == f["want"], (got, f["want"])
        if "again" in f:
            b.remove(0)
            b.set(0, **f["again"])
        try:
            b.process(np.zeros((1, 480), np.float32))
            assert lib.kq_device_count() > 0, "a call went through with no device"
        except kq.KqError as e:
            assert lib.kq_device_count() <= 0, str(e)
        b.close()
        for geometry, kw, why in f["refused"]:
            with pytest.raises(kq.KqError, match=why):
                make(geometry, **kw)
