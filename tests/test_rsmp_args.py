"""Argument checks of the rational resampler bank (kq_rsmp_*): every limit is refused with -1 / NULL and a reason that
names the function and the field before any HIP call, so they hold without a GPU (kq_rsmp_create, kq_rsmp_set and
kq_rsmp_remove touch no device); the rates, the delay and the output counts the bank reports; and the coefficients it
designs against the model's own design."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
import rsmp_model as rm
from ka9q_sdr_amd.resample import RsmpBank, RsmpConfig, RsmpInfo, RsmpParams, _bind, rsmp_params


@pytest.fixture(scope="module")
def lib():
    kq.build_library()
    return _bind(kq.load_library())


def _cfg(**kw):
    c = dict(device=0, in_rate_num=10000000, in_rate_den=256, out_rate=48000, taps=32, cutoff_hz=15000.0, kaiser_beta=3.0,
             max_slots=8, max_samples=1 << 14, stream=None)
    c.update(kw)
    return RsmpConfig(*c.values())


@pytest.fixture
def bank(lib):
    h = lib.kq_rsmp_create(C.byref(_cfg()))
    assert h, lib.kq_last_error()
    yield h
    assert lib.kq_rsmp_destroy(h) == 0


NAMES = {"kq_rsmp_create", "kq_rsmp_destroy", "kq_rsmp_set", "kq_rsmp_remove", "kq_rsmp_sync", "kq_rsmp_reset",
         "kq_rsmp_max_out", "kq_rsmp_get_info", "kq_rsmp_get_taps", "kq_rsmp_process"}


def test_symbols_exported_and_declared(lib):
    import test_abi
    decl = test_abi._declared("ka9q_hip.h")
    assert NAMES <= decl and {n for n in decl if n.startswith("kq_rsmp_")} == NAMES
    for n in sorted(NAMES):
        assert hasattr(lib, n), n
    assert kq.RsmpBank and kq.rsmp_params
    assert lib.kq_abi_version() == 6


def test_record_layouts():
    assert C.sizeof(RsmpParams) == 8 and C.sizeof(RsmpConfig) == 48 and C.sizeof(RsmpInfo) == 40
    assert RsmpConfig.max_samples.offset == 32 and RsmpConfig.stream.offset == 40
    assert RsmpInfo.delay_in_samples.offset == 16 and RsmpInfo.next_out.offset == 32


def test_null_config_refused(lib):
    assert lib.kq_rsmp_create(None) is None
    assert lib.kq_last_error() == b"kq_rsmp_create: null config"


def test_good_configs_accepted(lib):
    for kw in (dict(), dict(in_rate_num=8000, in_rate_den=1, out_rate=8000, cutoff_hz=3000.0),
               dict(in_rate_num=384000, in_rate_den=1, out_rate=384000),
               dict(in_rate_num=8000, in_rate_den=1, out_rate=128000, cutoff_hz=3000.0),      # 16 / 1
               dict(in_rate_num=384000, in_rate_den=1, out_rate=24000, cutoff_hz=10000.0),    # 1 / 16
               dict(in_rate_num=48000, in_rate_den=1, out_rate=44100, taps=64),               # 147 / 160
               dict(in_rate_num=12502, in_rate_den=1, out_rate=8192, cutoff_hz=3000.0, taps=64),   # P = 4096, P T = 2^18
               dict(taps=4), dict(taps=256), dict(kaiser_beta=0.0), dict(cutoff_hz=19531.0),
               dict(max_slots=65536), dict(max_samples=1 << 28), dict(max_samples=1)):
        h = lib.kq_rsmp_create(C.byref(_cfg(**kw)))
        assert h, (kw, lib.kq_last_error())
        assert lib.kq_rsmp_destroy(h) == 0


@pytest.mark.parametrize("kw,why", [
    (dict(in_rate_num=0), b"in_rate_num 0"),
    (dict(in_rate_den=0), b"in_rate_den 0"),
    (dict(in_rate_den=-1), b"in_rate_den -1"),
    (dict(in_rate_num=7999, in_rate_den=1), b"in_rate_num 7999 / in_rate_den 1 must be 8000..384000 Hz"),
    (dict(in_rate_num=384001, in_rate_den=1), b"in_rate_num 384001 / in_rate_den 1 must be 8000..384000 Hz"),
    (dict(in_rate_num=10000000, in_rate_den=2048), b"in_rate_num 10000000 / in_rate_den 2048"),     # 4882.8 Hz
    (dict(out_rate=7999), b"out_rate 7999 must be 8000..384000"),
    (dict(out_rate=384001), b"out_rate 384001 must be 8000..384000"),
    (dict(in_rate_num=8000, in_rate_den=1, out_rate=128001, cutoff_hz=3000.0), b"P / Q = 128001 / 8000, must be 1/16..16"),
    (dict(in_rate_num=384000, in_rate_den=1, out_rate=23999, cutoff_hz=3000.0), b"P / Q = 23999 / 384000, must be 1/16..16"),
    (dict(out_rate=48001), b"gives P = 96002 phases, 4096 at most"),
    (dict(in_rate_num=12500, in_rate_den=1, out_rate=8194, cutoff_hz=3000.0), b"gives P = 4097 phases, 4096 at most"),
    (dict(taps=3), b"taps 3 must be 4..256"),
    (dict(taps=257), b"taps 257 must be 4..256"),
    (dict(in_rate_num=12502, in_rate_den=1, out_rate=8192, cutoff_hz=3000.0, taps=65), b"taps 65 x P 4096 = 266240 coefficients"),
    (dict(cutoff_hz=0.0), b"cutoff_hz 0"),
    (dict(cutoff_hz=-1.0), b"cutoff_hz -1"),
    (dict(cutoff_hz=19531.25), b"cutoff_hz 19531.2 must be above 0 and below min(Fi, Fo) / 2 = 19531.2"),
    (dict(in_rate_num=192000, in_rate_den=1, cutoff_hz=24000.0), b"cutoff_hz 24000 must be above 0 and below min(Fi, Fo) / 2 = 24000"),
    (dict(cutoff_hz=float("nan")), b"cutoff_hz"),
    (dict(kaiser_beta=-1.0), b"kaiser_beta"),
    (dict(kaiser_beta=float("inf")), b"kaiser_beta"),
    (dict(kaiser_beta=float("nan")), b"kaiser_beta"),
    (dict(max_slots=0), b"max_slots 0"),
    (dict(max_slots=65537), b"max_slots 65537"),
    (dict(max_samples=0), b"max_samples 0"),
    (dict(max_samples=(1 << 28) + 1), b"max_samples 268435457"),
])
def test_bad_config_refused(lib, kw, why):
    assert lib.kq_rsmp_create(C.byref(_cfg(**kw))) is None
    msg = lib.kq_last_error()
    assert msg.startswith(b"kq_rsmp_create: ") and why in msg, msg


def test_set_and_remove_need_no_device(lib, bank):
    """set, set again, remove: host-side only; they take effect at the next process"""
    for slot, ch in ((0, 1), (7, 2), (0, 2), (3, 1)):
        assert lib.kq_rsmp_set(bank, slot, C.byref(rsmp_params(source=slot, channels=ch))) == 0, lib.kq_last_error()
    for slot in (0, 7, 3):
        assert lib.kq_rsmp_remove(bank, slot) == 0, lib.kq_last_error()
    assert lib.kq_rsmp_remove(bank, 3) == -1
    assert lib.kq_last_error() == b"kq_rsmp_remove: slot 3 holds no resampler"
    assert lib.kq_rsmp_sync(bank) == 0 and lib.kq_rsmp_reset(bank) == 0


def test_bad_params_and_slots_refused(lib, bank):
    for ch in (0, 3, -1):
        for h in (None, bank):   # checked before the bank is looked at
            assert lib.kq_rsmp_set(h, 0, C.byref(rsmp_params(channels=ch))) == -1
            assert lib.kq_last_error() == b"kq_rsmp_set: channels %d must be 1 or 2" % ch
    p = rsmp_params()
    assert lib.kq_rsmp_set(None, 65536, C.byref(p)) == -1
    assert b"kq_rsmp_set: slot 65536" in lib.kq_last_error()
    assert lib.kq_rsmp_set(bank, 8, C.byref(p)) == -1     # max_slots = 8
    assert lib.kq_last_error() == b"kq_rsmp_set: slot 8 >= max_slots 8"
    assert lib.kq_rsmp_set(bank, 0, None) == -1
    assert lib.kq_last_error() == b"kq_rsmp_set: null params"
    assert lib.kq_rsmp_set(None, 0, C.byref(p)) == -1
    assert lib.kq_last_error() == b"kq_rsmp_set: null bank"
    assert lib.kq_rsmp_remove(bank, 9) == -1
    assert lib.kq_last_error() == b"kq_rsmp_remove: slot 9 holds no resampler"
    assert lib.kq_rsmp_get_info(bank, None) == -1
    assert lib.kq_last_error() == b"kq_rsmp_get_info: null info"
    assert lib.kq_rsmp_get_taps(bank, None, 4) == -1
    assert lib.kq_last_error() == b"kq_rsmp_get_taps: null dst"


def test_bad_process_refused(lib, bank):
    buf = np.zeros(1 << 15, np.float32)
    out = np.zeros(1 << 15, np.float32)
    pcm = np.zeros(1 << 15, np.int16)

    def call(h, src, fmt, src_stride, row_stride, block_len, nblocks, o=None, ostride=0, p=None, pstride=0):
        return lib.kq_rsmp_process(h, src, fmt, src_stride, row_stride, block_len, nblocks, 0, o, ostride, p, pstride)
    assert call(bank, buf.ctypes.data, 0, 0, 4096, 4096, 5) == -1   # 20480 > 16384
    assert b"kq_rsmp_process: nblocks 5 x block_len 4096 = 20480 > max_samples 16384" in lib.kq_last_error()
    assert call(bank, buf.ctypes.data, 0, 0, 100, 200, 2) == -1
    assert b"kq_rsmp_process: row_stride 100 < block_len 200" in lib.kq_last_error()
    assert call(bank, buf.ctypes.data, 2, 0, 16, 16, 1) == -1         # KQ_PCM_S16: the modulator's
    assert b"kq_rsmp_process: unknown sample format 2" in lib.kq_last_error()
    # 625 samples at 768 / 625 give J = 768
    assert call(bank, buf.ctypes.data, 0, 0, 625, 625, 1, out.ctypes.data, 767) == -1
    assert b"kq_rsmp_process: out_stride 767 < 1 J = 768" in lib.kq_last_error()
    assert call(bank, buf.ctypes.data, 0, 0, 625, 625, 1, None, 0, pcm.ctypes.data, 767) == -1
    assert b"kq_rsmp_process: pcm_stride 767 < 1 J = 768" in lib.kq_last_error()
    assert call(bank, None, 0, 0, 16, 16, 1) == -1
    assert b"kq_rsmp_process: null src" in lib.kq_last_error()
    assert call(bank, None, 0, 0, 0, 0, 0) == 0        # nothing to do
    assert call(None, buf.ctypes.data, 0, 0, 16, 16, 1) == -1
    assert lib.kq_last_error() == b"kq_rsmp_process: null bank"
    # with a stereo slot set, a block is 2 block_len elements and the outputs 2 J
    assert lib.kq_rsmp_set(bank, 1, C.byref(rsmp_params(channels=2))) == 0
    assert call(bank, buf.ctypes.data, 0, 0, 300, 200, 2) == -1
    assert b"kq_rsmp_process: row_stride 300 < 400, a block of block_len 200 samples of a stereo slot" in lib.kq_last_error()
    assert call(bank, buf.ctypes.data, 0, 0, 1250, 625, 1, out.ctypes.data, 1535) == -1
    assert b"kq_rsmp_process: out_stride 1535 < 2 J = 1536" in lib.kq_last_error()


def test_without_a_slot_only_the_indices_move(lib, bank):
    """with no slot set, process succeeds, touches no device, and returns the J of the shared grid"""
    buf = np.zeros(1 << 14, np.float32)
    info = RsmpInfo()
    n = j = 0
    for s in (1, 1, 7, 1000, 16384, 1):
        want = rm.count(n, s, 768, 625)
        assert lib.kq_rsmp_process(bank, buf.ctypes.data, 0, 0, s, s, 1, 0, None, 0, None, 0) == want
        n, j = n + s, j + want
        assert lib.kq_rsmp_get_info(bank, C.byref(info)) == 0 and (info.next_in, info.next_out) == (n, j)
    assert j == rm.ceil_div(n * 768, 625)
    assert lib.kq_rsmp_sync(bank) == 0 and lib.kq_rsmp_reset(bank) == 0
    assert lib.kq_rsmp_get_info(bank, C.byref(info)) == 0 and (info.next_in, info.next_out) == (0, 0)


def test_null_handles_refused(lib):
    for fn, args in ((lib.kq_rsmp_destroy, ()), (lib.kq_rsmp_sync, ()), (lib.kq_rsmp_reset, ()), (lib.kq_rsmp_remove, (0,)),
                     (lib.kq_rsmp_get_info, (None,)), (lib.kq_rsmp_get_taps, (None, 0))):
        assert fn(None, *args) == -1
        assert b"null bank" in lib.kq_last_error()
    assert lib.kq_rsmp_max_out(None, 100) == 0
    assert lib.kq_last_error() == b"kq_rsmp_max_out: null bank"


# in_rate_num, in_rate_den, out_rate, T -> P, Q
RATES = [(10000000, 256, 48000, 32, 768, 625), (192000, 1, 48000, 96, 1, 4), (48000, 1, 44100, 48, 147, 160)]


@pytest.mark.parametrize("num,den,fo,T,P,Q", RATES)
def test_info_and_max_out(lib, num, den, fo, T, P, Q):
    assert rm.ratio(num, den, fo) == (P, Q)
    h = lib.kq_rsmp_create(C.byref(_cfg(in_rate_num=num, in_rate_den=den, out_rate=fo, taps=T)))
    assert h, lib.kq_last_error()
    info = RsmpInfo()
    assert lib.kq_rsmp_get_info(h, C.byref(info)) == 0
    assert (info.P, info.Q, info.taps, info.next_in, info.next_out) == (P, Q, T, 0, 0)
    assert info.delay_in_samples == (P * T - 1) / (2.0 * P)
    for n in (0, 1, 2, Q - 1, Q, Q + 1, 1000, 1 << 28):
        assert lib.kq_rsmp_max_out(h, n) == rm.ceil_div(n * P, Q)
        for n0 in (0, 1, 5, Q - 1, 17 << 28):
            assert rm.count(n0, n, P, Q) <= lib.kq_rsmp_max_out(h, n)
    assert lib.kq_rsmp_destroy(h) == 0


@pytest.mark.parametrize("kw", [dict(), dict(taps=5, cutoff_hz=9000.0), dict(in_rate_num=192000, in_rate_den=1, taps=96, cutoff_hz=20000.0),
                                dict(in_rate_num=48000, in_rate_den=1, out_rate=44100, taps=48, kaiser_beta=5.5),
                                dict(in_rate_num=200000, in_rate_den=4, taps=8, kaiser_beta=0.0),
                                dict(in_rate_num=12502, in_rate_den=1, out_rate=8192, cutoff_hz=3000.0, taps=64),
                                dict(in_rate_num=8000, in_rate_den=1, out_rate=12000, taps=4, cutoff_hz=2000.0)])
def test_taps_match_the_models_design(lib, kw):
    """g against the float64 design of tests/rsmp_model.py: within one ulp of float32, which is what can be promised -- the
    library sums the series of I0 itself and takes sin(pi t) / (pi t) from libm where numpy has np.i0 and np.sinc, so the
    doubles may differ in their last places and one of them may round to the neighbouring float.  In the cases here they
    do not: all 297 916 coefficients are equal to the last bit (the count is printed).  The GPU tests hand the bank's own
    taps to the model, so they do not lean on this."""
    c = _cfg(**kw)
    P, Q = rm.ratio(c.in_rate_num, c.in_rate_den, c.out_rate)
    K = P * c.taps
    h = lib.kq_rsmp_create(C.byref(c))
    assert h, lib.kq_last_error()
    g = np.zeros(K + 2, np.float32)
    assert lib.kq_rsmp_get_taps(h, g.ctypes.data, 2) == K and not g[2:].any()      # cap is kept
    assert lib.kq_rsmp_get_taps(h, g.ctypes.data, K + 2) == K and not g[K:].any()
    assert lib.kq_rsmp_destroy(h) == 0
    got = g[:K].reshape(P, c.taps)
    want = rm.design(P, c.taps, c.in_rate_num / c.in_rate_den, float(c.cutoff_hz), float(c.kaiser_beta))
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("rsmp taps %s: %d of %d differ, by at most %d ulp" % (kw, int((ulps > 0).sum()), K, int(ulps.max())))
    tiny = np.abs(want) < 1e-30      # (a zero crossing of the sinc: no ulp to speak of)
    assert ulps[~tiny].max() <= 1 and np.abs(got[tiny]).max(initial=0.0) < 1e-20
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() < 2e-2
    assert abs(got.astype(np.float64).sum() - P) < 1e-4 * P


def test_python_helpers():
    assert RsmpBank.clean_cutoff(39062.5, 48000, 32, 3.0) == rm.clean_cutoff(39062.5, 48000, 32, 3.0)
    assert abs(RsmpBank.transition_hz(50000.0, 32, 3.0) - 2 * 50000 * 10 ** 0.5 / 32) < 1e-9
    b = RsmpBank(10000000, 256, 48000, 32, 15000.0, 3.0, 4, 1000)
    assert (b.P, b.Q, b.T, b.max_out(625), b.tile) == (768, 625, 32, 768, 1024)
    assert b.taps().shape == (768, 32)
    b.set(2, source=1, channels=2)
    b.remove(2)
    b.close()
