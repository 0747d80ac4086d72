"""GPU raw A/D conditioning (kq_fe_*) against its definition (tests/fe_model.py: exact), bit for bit, and the fused
kq_fe_process_decim against kq_fe_process followed by kq_decim_process."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "oracle"), HERE]
import fe_model as fm  # noqa: E402
import kq_oracle as ko  # noqa: E402

pytestmark = pytest.mark.gpu

FLOATS = ("DC_i", "DC_q", "imbalance", "sinphi", "in_power", "gain_i", "gain_q", "secphi", "tanphi")


def _rates(block):
    """estimator constants fast enough that every block moves the state visibly: r = 0.05, dc_alpha * block = 0.1"""
    return dict(adc_samprate=20.0 * block, dc_alpha=0.1 / block, power_alpha=1.0)


def _same_status(rec, want, what):
    for k in ("samples", "blocks", "clips"):
        assert int(rec[k]) == int(want[k]), (what, k, int(rec[k]), int(want[k]))
    for k in FLOATS:
        a, b = np.float32(rec[k]).view(np.uint32), np.float32(want[k]).view(np.uint32)
        assert a == b, (what, k, float(rec[k]), float(want[k]))


def _same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), what


@pytest.mark.parametrize("fmt,block", [(fm.S8, 4096), (fm.S8, 1000), (fm.S8, 64), (fm.S8, 131072), (fm.S16, 4096),
                                       (fm.S16, 1000), (fm.S16, 64), (fm.S16, 6001)])
def test_process_matches_the_definition(gpu, fmt, block):
    """cf32, int16, every block_status record and the final status, over ragged calls: one sample, less than a
    block, several blocks and a remainder, and a long one."""
    from ka9q_sdr_amd import FrontEnd
    calls = [1, block // 2 + 3, 3 * block + 77, 7, 40 * block + 5 if block <= 6001 else 2 * block + 5]
    raw = fm.make_raw(fmt, sum(calls), seed=block + fmt)
    if fmt == fm.S8:
        raw[5::97, 0] = -128    # the -128 rule, I and Q
        raw[11::89, 1] = -128
    kw = _rates(block)
    fe = FrontEnd(fmt, block, max_samples=max(calls), **kw)
    model = fm.Exact(fmt, block, kw["adc_samprate"], kw["dc_alpha"], kw["power_alpha"])
    pos = 0
    for c, n in enumerate(calls):
        y, s16, st = fe.process(raw[pos:pos + n], want_cf32=True, want_s16=True)
        wy, ws16, wst = model.process(raw[pos:pos + n])
        _same_bits(y, wy, "call %d" % c)
        assert np.array_equal(s16, ws16), "call %d" % c
        assert len(st) == len(wst), (c, len(st), len(wst))
        for b in range(len(wst)):
            _same_status(st[b], wst[b], "call %d block %d" % (c, b))
        _same_status(fe.status(), model.st, "after call %d" % c)
        pos += n
    assert int(fe.status()["blocks"]) == sum(calls) // block
    # either output alone
    y, s16, _ = fe.process(raw[:100], want_cf32=False, want_s16=True)
    assert y is None and np.array_equal(s16, model.process(raw[:100])[1])
    fe.close()


@pytest.mark.parametrize("fmt", [fm.S8, fm.S16])
def test_call_boundaries_do_not_matter(gpu, fmt):
    from ka9q_sdr_amd import FrontEnd
    block = 3000
    raw = fm.make_raw(fmt, 50 * block + 1234, seed=77)
    kw = _rates(block)
    one = FrontEnd(fmt, block, max_samples=len(raw), **kw)
    y, s16, st = one.process(raw, want_s16=True)
    cut = FrontEnd(fmt, block, max_samples=len(raw), **kw)
    rng = np.random.default_rng(3)
    ys, ss, sts = [], [], []
    pos = 0
    while pos < len(raw):
        n = int(rng.choice([1, 2, 9, 2999, 3000, 3001, 12345, 40000]))
        a, b, c = cut.process(raw[pos:pos + n], want_s16=True)
        ys.append(a), ss.append(b), sts.append(c)
        pos += n
    _same_bits(np.concatenate(ys), y, "samples")
    assert np.array_equal(np.concatenate(ss), s16)
    assert np.concatenate(sts).tobytes() == st.tobytes()
    assert cut.status().tobytes() == one.status().tobytes()
    one.close()
    cut.close()


@pytest.mark.parametrize("fmt", [fm.S8, fm.S16])
@pytest.mark.parametrize("log_dec,thr,offset,block", [(1, 8, 0, 1000), (1, 0, 1, 64), (6, 8, 1, 5000), (6, 3, 0, 5000),
                                                      (6, 8, 1, 131072), (7, 5, 1, 1000), (7, 8, 0, 4096)])
def test_fused_cascade_is_the_two_calls(gpu, fmt, log_dec, thr, offset, block):
    """kq_fe_process_decim == kq_fe_process into a buffer, then kq_decim_process on it, both from fresh handles:
    outputs, int16 and the carried state over four ragged calls.  block 1000 / 5000: the cascade's 4096-sample tiles
    straddle block boundaries."""
    from ka9q_sdr_amd import Decimator, FrontEnd
    n_outs = [700, 1, 513, 64]
    kw = _rates(block)
    max_samples = max(n_outs) << log_dec
    fused = FrontEnd(fmt, block, max_samples=max_samples, decimator=dict(log_decimate=log_dec, stage_threshold=thr,
                                                                          offset=offset), **kw)
    fe = FrontEnd(fmt, block, max_samples=max_samples, **kw)
    dec = Decimator(log_dec, thr, offset, max_out=max(n_outs))
    model = fm.Exact(fmt, block, kw["adc_samprate"], kw["dc_alpha"], kw["power_alpha"])
    oracle = ko.FrontEndDecimator(log_dec, thr, offset)
    for c, n_out in enumerate(n_outs):
        raw = fm.make_raw(fmt, n_out << log_dec, seed=200 + c, tone=0.2)
        y, s16, e, st = fused.process_decim(raw)
        x, _, wst = fe.process(raw)
        wy, ws16, we = dec.process(x)
        _same_bits(y, wy, "call %d" % c)
        assert np.array_equal(s16, ws16), "call %d" % c
        np.testing.assert_allclose(e, we, rtol=2e-6)
        assert st.tobytes() == wst.tobytes(), "call %d" % c
        assert fused.status().tobytes() == fe.status().tobytes()
        # and both are the definition followed by the oracle's cascade
        oy, _, _ = oracle.process(model.process(raw)[0])
        _same_bits(y, oy, "call %d against the models" % c)
    fused.close()
    fe.close()
    dec.close()


def test_reset_restores_the_initial_state(gpu):
    from ka9q_sdr_amd import FrontEnd
    block = 2048
    fe = FrontEnd(fm.S8, block, max_samples=1 << 16, decimator=dict(log_decimate=3), **_rates(block))
    raw = fm.make_raw(fm.S8, 5 * block + 8 * 100, seed=4)
    y, _, st = fe.process(raw)
    d1 = fe.process_decim(raw)
    assert int(fe.status()["blocks"]) == (2 * len(raw)) // block
    fe.reset()
    init = fm._initial()
    _same_status(fe.status(), init, "after reset")
    y2, _, st2 = fe.process(raw)
    _same_bits(y2, y, "after reset")
    assert st2.tobytes() == st.tobytes()
    fe.reset()
    d2 = fe.process_decim(raw)
    # the first pass ran the cascade on the stream's second copy: only the fresh start is compared
    fresh = FrontEnd(fm.S8, block, max_samples=1 << 16, decimator=dict(log_decimate=3), **_rates(block))
    d3 = fresh.process_decim(raw)
    _same_bits(d2[0], d3[0], "cascade after reset")
    assert d2[3].tobytes() == d3[3].tobytes() and d1[0].shape == d2[0].shape
    fe.close()
    fresh.close()


def test_mismatched_stream_is_refused(gpu):
    from ka9q_sdr_amd import Decimator, FrontEnd, KqError
    fe = FrontEnd(fm.S8, 4096, 1e6, max_samples=1 << 14)
    dec = Decimator(3, max_out=1 << 11)   # a private stream of its own
    raw = fm.make_raw(fm.S8, 1 << 14, seed=1)
    with pytest.raises(KqError, match="same device and stream"):
        fe.process_decim(raw, decimator=dec)
    assert int(fe.status()["blocks"]) == 0   # nothing ran
    ok = Decimator(3, max_out=1 << 11, stream=fe.stream)
    y, _, _, st = fe.process_decim(raw, decimator=ok)
    assert len(y) == 1 << 11 and len(st) == 4
    for h in (fe, dec, ok):
        h.close()


def test_device_resident_chain_feeds_bank(gpu):
    """Raw int8 on the device -> kq_fe_process_decim -> Bank.push_iq_device, nothing through the host: the audio equals
    the same bank fed from the host with the models' output."""
    import ctypes as C
    from ka9q_sdr_amd import Bank, FrontEnd, FE_STATUS_DTYPE, channel_config, KQ_FM_DEMOD
    hip = C.CDLL("libamdhip64.so")  # the runtime libka9q_hip.so is already bound to
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    log_dec, L, M, D = 3, 7680, 513, 8
    nblk = 4
    n_out = L * nblk
    n = n_out << log_dec
    block = 50000
    t = np.arange(n)
    sig = 0.5 * np.exp(2j * np.pi * (0.01 / 8) * t + 1j * 0.3 * np.sin(2 * np.pi * 1e-5 * t))
    rng = np.random.default_rng(11)
    sig = sig + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.stack([np.round(127 * (sig.real + 0.02)), np.round(127 * (1.1 * sig.imag - 0.01))], axis=1)
    raw = np.clip(raw, -128, 127).astype(np.int8)
    kw = _rates(block)
    fe = FrontEnd(fm.S8, block, max_samples=n, decimator=dict(log_decimate=log_dec, stage_threshold=8, offset=0), **kw)
    nst = n // block + 2
    raw_d, y_d, st_d = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(raw_d), raw.nbytes) == 0
    assert hip.hipMalloc(C.byref(y_d), 8 * n_out) == 0
    assert hip.hipMalloc(C.byref(st_d), 64 * nst) == 0
    assert hip.hipMemcpy(raw_d, raw.ctypes.data, raw.nbytes, 1) == 0
    done = fe.process_decim_device(raw_d, n_out, y_d, status_ptr=st_d)
    fe.sync()
    assert done == n // block
    model = fm.Exact(fm.S8, block, kw["adc_samprate"], kw["dc_alpha"], kw["power_alpha"])
    x, _, wst = model.process(raw)
    wy, _, _ = ko.FrontEndDecimator(log_dec, 8, 0).process(x)
    y = np.empty(n_out, np.complex64)
    st = np.zeros(nst, FE_STATUS_DTYPE)
    assert hip.hipMemcpy(y.ctypes.data, y_d, y.nbytes, 2) == 0
    assert hip.hipMemcpy(st.ctypes.data, st_d, st.nbytes, 2) == 0
    _same_bits(y, wy, "decimated samples")
    for b in range(done):
        _same_status(st[b], wst[b], "block %d" % b)
    bank = Bank(192000, L, M, D, max_channels=1, max_blocks=nblk)
    ch = bank.add_channel(channel_config(KQ_FM_DEMOD, -8000, 8000, second_lo=-0.01 * 192000))
    bank.push_iq_device(y_d, n_out)
    assert bank.process() == nblk
    bank.sync()
    ref = Bank(192000, L, M, D, max_channels=1, max_blocks=nblk)
    ref.add_channel(channel_config(KQ_FM_DEMOD, -8000, 8000, second_lo=-0.01 * 192000))
    ref.push_iq(wy)
    ref.process()
    ref.sync()
    for b in range(nblk):
        assert np.array_equal(bank.audio(ch, b), ref.audio(0, b))
    assert np.abs(bank.audio(ch, nblk - 1)).max() > 0
    for h in (fe, bank, ref):
        h.close()
    for p in (raw_d, y_d, st_d):
        hip.hipFree(p)
