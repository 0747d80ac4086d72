"""The rational resampler bank (kq_rsmp_*, ka9q_sdr_amd/csrc/kq_rsmp.hip) on the GPU against the float64 model of
tests/rsmp_model.py.  For every output |out - model| <= (T + 2) 2^-24 sum |g x|: the forward error bound of the defined
T-step fmaf fold (each step rounds once, relative error 2^-24 of a partial sum that sum |g x| bounds), with 2 to spare, as
mon_model.bound is derived; pcm is scaleclip of the call's own out, word for word; rows of empty slots and the padding
keep their fill.  The model runs on the bank's own coefficients (kq_rsmp_get_taps; tests/test_rsmp_args.py holds them to
the model's design), so the comparison is of the arithmetic alone."""
import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
import rsmp_model as rm
from ka9q_sdr_amd.resample import RsmpBank
from test_rsmp_model import CARRIERS, GEOM, PER_CALL, RSMP_BETA, RSMP_T, SPLITS, fm_afsk_case, fm_plan

pytestmark = pytest.mark.gpu

FILL_F, FILL_W = np.float32(7.25), np.int16(0x5a5a)
PAD = 3
# in_rate_num, in_rate_den, out_rate, T -> P / Q: 24/25, 768/625, 1/4 (P = 1), 3/2, 1/16
RATIOS = [(50000, 1, 48000, 8), (10000000, 256, 48000, 5), (192000, 1, 48000, 16), (8000, 1, 12000, 4), (384000, 1, 24000, 64)]


def _bank(num, den, fo, T, max_slots, max_samples):
    return RsmpBank(num, den, fo, T, 0.4 * min(num / den, fo), 2.0, max_slots, max_samples)


def _layout(S):
    """slot -> (source row, channels): slot numbers with gaps, rows shared, every fourth slot stereo; and the rows"""
    if S == 1:
        return {2: (1, 1)}, 3
    rows = max(2, (S * 3) // 5)
    return {s + s // 3: ((7 * s) % rows, 2 if s % 4 == 1 else 1) for s in range(S)}, rows


def _input(rng, rows, bl, nblocks, fmt):
    """[rows][nblocks][2 bl + PAD]: every block wide enough for a stereo reader, junk in the padding"""
    shape = (rows, nblocks, 2 * bl + PAD)
    if fmt == kq.KQ_PCM_S16BE:
        w = rng.integers(-32768, 32768, shape).astype(">i2")
        w[:, :, 2 * bl:] = -32768
        return w
    x = (0.6 * rng.standard_normal(shape)).astype(np.float32)
    x[:, :, 2 * bl:] = np.nan
    return x


def _side(buf, row, ch, side, bl):
    """what a slot of ch sides on `row` reads of the call, one side, as float32"""
    blocks = buf[row, :, :ch * bl]
    v = rm.from_s16be(blocks) if buf.dtype.itemsize == 2 else blocks
    return v.reshape(-1, ch)[:, side]


def _call(bank, buf, bl, nblocks, device, c):
    """one kq_rsmp_process on `buf` from host or device memory -> (J, out, pcm) [max_slots][c J + PAD], pcm in host order"""
    fmt = kq.KQ_PCM_S16BE if buf.dtype.itemsize == 2 else kq.KQ_PCM_F32
    rows, _, rs = buf.shape
    i = bank.info()
    J = rm.count(i.next_in, bl * nblocks, bank.P, bank.Q)
    w = c * J + PAD
    out = np.full((bank.max_slots, w), FILL_F, np.float32)
    pcm = np.full((bank.max_slots, w), FILL_W, np.int16)
    raw = np.ascontiguousarray(buf).view(np.int16 if buf.dtype.itemsize == 2 else np.float32)
    if device:
        t_in, t_out, t_pcm = torch.from_numpy(raw).cuda(), torch.from_numpy(out).cuda(), torch.from_numpy(pcm).cuda()
        torch.cuda.synchronize()
        got = bank.process_device(t_in.data_ptr(), fmt, nblocks * rs, rs, bl, nblocks, t_out.data_ptr(), w, t_pcm.data_ptr(), w)
        bank.sync()
        out, pcm = t_out.cpu().numpy(), t_pcm.cpu().numpy()
    else:
        got = bank._chk(bank.lib.kq_rsmp_process(bank.h, raw.ctypes.data, fmt, nblocks * rs, rs, bl, nblocks, 0, out.ctypes.data, w,
                                                 pcm.ctypes.data, w), "kq_rsmp_process")
    assert got == J
    i2 = bank.info()
    assert (i2.next_in, i2.next_out) == (i.next_in + bl * nblocks, i.next_out + J)
    return J, out, pcm.view(">i2").astype(np.int16)


def _models(bank, layout, start=0):
    g = bank.taps()
    return {s: [rm.RsmpModel(bank.P, bank.Q, g, start) for _ in range(ch)] for s, (_, ch) in layout.items()}


def _check(bank, models, layout, buf, bl, J, out, pcm, c, what):
    """every active slot against its models (which take the call's samples), everything else against the fill"""
    worst = 0.0
    written = np.zeros(out.shape, bool)
    for s, (row, ch) in layout.items():
        for side in range(ch):
            y, ab = models[s][side].feed(_side(buf, row, ch, side, bl))
            assert len(y) == J
            got = out[s, side:ch * J:ch]
            err = np.abs(got.astype(np.float64) - y)
            lim = rm.bound(bank.T) * ab
            assert np.all(err <= lim), (what, s, side, float(np.max(err - lim)))
            worst = max(worst, float(np.max(err / np.maximum(lim, 1e-300), initial=0.0)))
        written[s, :ch * J] = True
        assert np.array_equal(pcm[s, :ch * J], rm.scaleclip(out[s, :ch * J])), (what, s)
    assert np.all(out[~written] == FILL_F) and np.all(pcm[~written] == FILL_W), what
    return worst


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("num,den,fo,T", RATIOS)
def test_parity_from_host_and_device_memory(gpu, num, den, fo, T, S):
    """three calls -- 96 samples as three blocks in padded rows, 5 samples, 1 sample (at 1/4 it gives no output) -- from host
    and device memory, float and big-endian int16"""
    layout, rows = _layout(S)
    c = 2 if any(ch == 2 for _, ch in layout.values()) else 1
    worst = 0.0
    for device in (False, True):
        for fmt in (kq.KQ_PCM_F32, kq.KQ_PCM_S16BE):
            rng = np.random.default_rng(5)
            bank = _bank(num, den, fo, T, max(layout) + 3, 96)
            for s, (row, ch) in layout.items():
                bank.set(s, source=row, channels=ch)
            models = _models(bank, layout)
            for bl, nblocks in ((32, 3), (5, 1), (1, 1)):
                buf = _input(rng, rows, bl, nblocks, fmt)
                J, out, pcm = _call(bank, buf, bl, nblocks, device, c)
                worst = max(worst, _check(bank, models, layout, buf, bl, J, out, pcm, c, (device, fmt, bl, nblocks)))
            if (bank.P, bank.Q) == (1, 4):
                assert J == 0
            bank.close()
    print("rsmp parity %d/%d T = %d, %d slots: worst error %.3f of the bound" % (bank.P, bank.Q, T, S, worst))


@pytest.mark.parametrize("num,den,fo,T,bl,nblocks", [(50000, 1, 48000, 8, 600, 4), (384000, 1, 24000, 64, 6400, 2)])
@pytest.mark.parametrize("device", [False, True])
def test_several_tiles_and_a_block_boundary_inside_one(gpu, num, den, fo, T, bl, nblocks, device):
    layout, rows = _layout(3)
    bank = _bank(num, den, fo, T, 8, bl * nblocks)
    J = rm.count(0, bl * nblocks, bank.P, bank.Q)
    assert J >= 2 * bank.tile + 1                               # three tiles and more
    assert any(0 < (k * bl * bank.P // bank.Q) % bank.tile for k in range(1, nblocks))
    for s, (row, ch) in layout.items():
        bank.set(s, source=row, channels=ch)
    models = _models(bank, layout)
    buf = _input(np.random.default_rng(6), rows, bl, nblocks, kq.KQ_PCM_F32)
    got, out, pcm = _call(bank, buf, bl, nblocks, device, 2)
    assert got == J
    _check(bank, models, layout, buf, bl, J, out, pcm, 2, (num, T))
    bank.close()


def _stream_run(bank, layout, x, xm, sizes, device):
    """x [rows][n][2] (rows of pairs) and, as the row after them, xm [n] (a mono row) through calls of `sizes`; -> per slot
    the concatenated out and pcm"""
    outs = {s: [] for s in layout}
    pcms = {s: [] for s in layout}
    at = 0
    for n in sizes:
        buf = np.full((x.shape[0] + 1, 1, 2 * n + PAD), np.nan, np.float32)
        buf[:-1, 0, :2 * n] = x[:, at:at + n].reshape(x.shape[0], 2 * n)
        buf[-1, 0, :n] = xm[at:at + n]
        J, out, pcm = _call(bank, buf, n, 1, device, 2)
        for s, (_, ch) in layout.items():
            outs[s].append(out[s, :ch * J].copy())
            pcms[s].append(pcm[s, :ch * J].copy())
        at += n
    assert at == x.shape[1]
    return {s: np.concatenate(v) for s, v in outs.items()}, {s: np.concatenate(v) for s, v in pcms.items()}


def test_call_splits_change_nothing(gpu):
    """the same stream as one call and as calls of 1, 1, 7, 100, 1, 3 and the rest, from host and device memory: the same
    bits in out and pcm.  (A mono slot on a row of pairs would read the first half of each call's pairs, another stream
    under another split: the mono slot here has a row of its own.)"""
    N = 2400
    layout = {0: (0, 2), 3: (1, 2), 4: (0, 2), 5: (2, 1)}
    rng = np.random.default_rng(8)
    x = (0.7 * rng.standard_normal((2, N, 2))).astype(np.float32)
    xm = (0.7 * rng.standard_normal(N)).astype(np.float32)
    x[1, 40, 0], x[1, 900, 1] = np.nan, np.inf                 # they propagate the same way under every split
    runs = []
    for sizes in ((N,), SPLITS + (N - sum(SPLITS),)):
        for device in (False, True):
            bank = _bank(10000000, 256, 48000, 5, 6, N)
            for s, (row, ch) in layout.items():
                bank.set(s, source=row, channels=ch)
            runs.append(_stream_run(bank, layout, x, xm, sizes, device))
            bank.close()
    o0, p0 = runs[0]
    assert len(o0[0]) == 2 * rm.ceil_div(N * 768, 625) and len(o0[5]) == rm.ceil_div(N * 768, 625)
    assert np.isnan(o0[3]).sum() >= 5 and np.array_equal(o0[0], o0[4])
    for o, p in runs[1:]:
        for s in layout:
            assert np.array_equal(o0[s].view(np.int32), o[s].view(np.int32)), s
            assert np.array_equal(p0[s], p[s]), s


def test_set_remove_and_reset_midstream(gpu):
    """a slot set after two calls starts on the shared grid with zero history; a removed slot's rows stop changing; reset
    reproduces the first run's bits"""
    num, den, fo, T = 10000000, 256, 48000, 5
    rng = np.random.default_rng(9)
    bank = _bank(num, den, fo, T, 6, 200)
    first = {0: (0, 1), 1: (1, 2)}
    for s, (row, ch) in first.items():
        bank.set(s, source=row, channels=ch)
    models = _models(bank, first)
    bufs = [_input(rng, 2, bl, nb, kq.KQ_PCM_F32) for bl, nb in ((50, 2), (37, 1), (60, 3), (11, 1))]
    shapes = [(50, 2), (37, 1), (60, 3), (11, 1)]
    run1 = []
    for buf, (bl, nb) in zip(bufs[:2], shapes[:2]):
        J, out, pcm = _call(bank, buf, bl, nb, True, 2)
        _check(bank, models, first, buf, bl, J, out, pcm, 2, "first run")
        run1.append((out, pcm))
    # slot 3 joins at n = 137: zero history, the shared grid's phase
    n_set = bank.info().next_in
    assert n_set == 137
    bank.set(3, source=0, channels=1)
    layout = dict(first)
    layout[3] = (0, 1)
    models[3] = _models(bank, {3: (0, 1)}, start=n_set)[3]
    bl, nb = shapes[2]
    J, out, pcm = _call(bank, bufs[2], bl, nb, True, 2)
    _check(bank, models, layout, bufs[2], bl, J, out, pcm, 2, "slot 3 set")
    # slot 1 leaves: its rows keep the fill from then on (_check holds everything unwritten to it)
    bank.remove(1)
    del layout[1]
    bl, nb = shapes[3]
    J, out, pcm = _call(bank, bufs[3], bl, nb, False, 1)
    _check(bank, models, layout, bufs[3], bl, J, out, pcm, 1, "slot 1 removed")
    # reset: n and j at 0, zero history; the first run's slots give the first run's bits
    bank.reset()
    bank.remove(3)
    bank.set(1, source=1, channels=2)
    for (o1, p1), buf, (bl, nb) in zip(run1, bufs[:2], shapes[:2]):
        J, out, pcm = _call(bank, buf, bl, nb, True, 2)
        assert np.array_equal(out.view(np.int32), o1.view(np.int32)) and np.array_equal(pcm, p1)
    bank.close()


def test_indices_beyond_32_bits(gpu):
    """17 idle calls of 2^28 samples, then a slot and 200 samples at 768 / 625: the model started at n0 = 17 2^28"""
    big = 1 << 28
    bank = _bank(10000000, 256, 48000, 32, 2, big)
    dummy = np.zeros(4, np.float32)
    j = 0
    for k in range(17):
        J = rm.count(k * big, big, 768, 625)
        assert bank.lib.kq_rsmp_process(bank.h, dummy.ctypes.data, kq.KQ_PCM_F32, 0, big, big, 1, 0, None, 0, None, 0) == J
        j += J
    i = bank.info()
    assert (i.next_in, i.next_out) == (17 * big, j) and i.next_in * 768 > 1 << 41
    layout = {1: (0, 1)}
    bank.set(1, source=0, channels=1)
    models = _models(bank, layout, start=17 * big)
    rng = np.random.default_rng(10)
    for device, (bl, nb) in ((True, (100, 2)), (False, (3, 1))):
        buf = _input(rng, 1, bl, nb, kq.KQ_PCM_F32)
        J, out, pcm = _call(bank, buf, bl, nb, device, 1)
        _check(bank, models, layout, buf, bl, J, out, pcm, 1, "beyond 2^32")
    bank.close()


def test_in_place_behind_a_receiver_bank(gpu):
    """Two flat FM channels of a receiver bank at 50 kHz carry AFSK-1200; the resampler runs on the bank's stream from its device
    audio plane, and its out goes to kq_afsk_push on the device: every frame sent comes back byte for byte, and out is bit
    for bit what a twin bank makes of the same plane pulled to the host.  (tests/test_rsmp_model.py holds the same chain
    through the oracle's receiver and the model.)"""
    from common import bank_cfg
    from ka9q_sdr_amd import AfskBank
    iq, sent, nblocks = fm_afsk_case()
    L, nch = GEOM["L"], len(CARRIERS)
    rx = kq.Bank(GEOM["samprate"], L, GEOM["M"], GEOM["D"], nch, PER_CALL)
    for p in fm_plan():
        rx.add_channel(bank_cfg(p))
    ncall = PER_CALL * rx.olen
    rs = RsmpBank.beside(rx, 48000, RSMP_T, max_slots=nch, kaiser_beta=RSMP_BETA)
    assert (rs.P, rs.Q) == (24, 25)
    twin = RsmpBank(GEOM["samprate"], GEOM["D"], 48000, RSMP_T, RsmpBank.clean_cutoff(50000.0, 48000, RSMP_T, RSMP_BETA), RSMP_BETA,
                    nch, ncall)
    afsk = AfskBank(nch, max_frames=8, stream=rs.stream)
    for b in (rs, twin):
        for s in range(nch):
            b.set(s, source=s, channels=1)
    width = rs.max_out(ncall) + 8
    out = torch.zeros((nch, width), dtype=torch.float32, device="cuda")
    for c in range(nblocks // PER_CALL):
        rx.push_iq(iq[c * PER_CALL * L:(c + 1) * PER_CALL * L])
        assert rx.process() == PER_CALL
        J = rs.process_bank(rx, out)
        afsk.push_device(out.data_ptr(), J, width)
        plane = np.array([np.concatenate([rx.audio(ch, b) for b in range(PER_CALL)]) for ch in range(nch)])
        tJ, tout, _ = twin.process(plane, want_pcm=False)
        assert tJ == J
        assert np.array_equal(out[:, :J].cpu().numpy().view(np.int32), tout[:nch, :J].view(np.int32)), c
    afsk.sync()
    for s in range(nch):
        assert afsk.frames(s) == sent[s], s
    for h in (afsk, rs, twin, rx):
        h.close()
