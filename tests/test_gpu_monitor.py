"""The monitor mixer bank (kq_mon_*) on the device against its float64 model (tests/mon_model.py): parity at the forward
error bound of the defined summation, bits independent of the call split and of the other buses, changes mid-stream, a
receiver bank's audio plane mixed in place, and a call of more than one time tile."""
import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.monitor import KQ_MON_F32, KQ_MON_S16BE, MonBank, pcm_array, status_array
import mon_model as mm

pytestmark = pytest.mark.gpu

RATE, H = 48000, 48
PANS = [-1.0, 0.0, 1.0, 1.0 / H, (H - 1.0) / H, -1.0 / H, -(H - 1.0) / H, 0.5, -0.25]   # delays 0, 1, H - 1 and H on either side


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _call_rows(x, stereo, col, T, nb, s16, pad=3):
    """frames col .. col + T - 1 of x [rows][n][2] as a call's input [rows][nb row_stride]: nb blocks, row_stride = 2 block_len
    + pad, a mono row's block block_len values (x[..., 0]), a stereo row's 2 block_len interleaved"""
    bl = T // nb
    rs = 2 * bl + pad
    a = np.zeros((x.shape[0], nb * rs), np.float32)
    for r in range(x.shape[0]):
        for k in range(nb):
            seg = x[r, col + k * bl:col + (k + 1) * bl]
            v = seg.reshape(-1) if stereo[r] else seg[:, 0]
            a[r, k * rs:k * rs + v.size] = v
    return (mm.to_s16be(a) if s16 else a), bl, rs


def _process(bank, a, bl, nb, rs, device):
    """one call, from host or from device memory -> out float32 [B][T][2], pcm int16 [B][T][2] (host order), status [B]"""
    if not device:
        return bank.process(a, bl, nb, rs)
    T, B = bl * nb, bank.max_buses
    s16 = a.dtype.itemsize == 2
    da = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if s16 else a).cuda()
    do = torch.full((B, T, 2), 7.0, dtype=torch.float32, device="cuda")
    dp = torch.full((B, T, 2), 7, dtype=torch.int16, device="cuda")
    ds = torch.full((B, 5), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert bank.process_device(da.data_ptr(), KQ_MON_S16BE if s16 else KQ_MON_F32, a.shape[1], rs, bl, nb, do.data_ptr(), 2 * T,
                               dp.data_ptr(), 2 * T, ds.data_ptr()) == T
    bank.sync()
    return do.cpu().numpy(), pcm_array(dp), status_array(ds)


def _check(out, pcm, st, want, absum, nsess, active, worst):
    """one call's outputs against the model and against each other; returns the worst error as a share of the bound"""
    for b in range(out.shape[0]):
        K = int(nsess[b])
        lim = mm.bound(K) * absum[b]
        err = np.abs(out[b].astype(np.float64) - want[b])
        assert np.all(err <= lim), (b, K, float((err - lim).max()))
        if K:
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()) if np.any(lim > 0) else 0.0)
        else:
            assert not _bits(out[b]).any() and not pcm[b].any()
        assert np.array_equal(pcm[b], mm.scaleclip(out[b])), b       # word for word, of the call's own out
        assert st["clipped"][b] == np.count_nonzero((pcm[b] == 32767) | (pcm[b] == -32768))
        assert st["sessions"][b] == K and st["active"][b] == active[b], (b, st[b], K, active[b])
        assert st["peak_left"][b] == np.abs(out[b, :, 0]).max() and st["peak_right"][b] == np.abs(out[b, :, 1]).max()
    return worst


def _sessions(K, rng, nbuses=1):
    """K sessions in odd slots, sources a permutation of the rows, every third stereo, pans through PANS then random, gains
    0 .. 2; the first is loud enough to clip"""
    src = rng.permutation(K)
    out = {}
    for k in range(K):
        pan = PANS[k] if k < len(PANS) else float(rng.uniform(-1, 1))
        out[2 * k + 1] = dict(source=int(src[k]), bus=k % nbuses if nbuses > 1 else 0, channels=2 if k % 3 == 1 else 1,
                              gain=2.0 if k == 0 else float(rng.uniform(0, 2)), pan=pan)
    return out


def _stereo_rows(sessions, rows):
    st = np.zeros(rows, bool)
    for p in sessions.values():
        st[p["source"]] |= p["channels"] == 2
    return st


def _both(samprate, max_sessions, nbuses, max_samples, sessions):
    bank, model = MonBank(samprate, max_sessions, nbuses, max_samples), mm.MonModel(samprate, nbuses)
    for slot, p in sessions.items():
        bank.set(slot, **p)
        model.set(slot, **p)
    return bank, model


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_parity_with_the_model(gpu, K, device, s16):
    """|out - model| <= (min(K, 64) + ceil(K / 64) + 2) 2^-24 sum |g x| per output sample, three calls of which two are shorter
    than the history; pcm, clip count, peaks, K and the count of sounding members from the call's own out, exactly"""
    rng = np.random.default_rng(100 + K)
    sessions = _sessions(K, rng)
    x = rng.uniform(-1, 1, (K, 102, 2))
    x[sessions[1]["source"]] = np.sign(x[sessions[1]["source"]]) * 0.999       # loud: gain 2 at pan -1 clips the left side
    if K > 2:
        x[sessions[5]["source"]] = 0.0                                           # a silent member
    stereo = _stereo_rows(sessions, K)
    bank, model = _both(RATE, 2 * K + 2, 1, 96, sessions)
    worst, col, clipped = 0.0, 0, 0
    for T, nb in ((96, 3), (5, 1), (1, 1)):
        a, bl, rs = _call_rows(x, stereo, col, T, nb, s16)
        out, pcm, st = _process(bank, a, bl, nb, rs, device)
        worst = _check(out, pcm, st, *model.process(a, bl, nb, rs), worst)
        assert T < 96 or st["active"][0] == (K - 1 if K > 2 else K)
        clipped += int(st["clipped"][0])
        col += T
    bank.close()
    assert clipped > 0
    print("mixer parity K %d %s %s: worst error %.3f of the bound" % (K, "device" if device else "host", "s16be" if s16 else "f32", worst))


def _run_split(sessions, x, stereo, calls, nbuses, device=False, s16=False, max_sessions=160):
    bank = MonBank(RATE, max_sessions, nbuses, max(T for T, _ in calls))
    for slot, p in sessions.items():
        bank.set(slot, **p)
    outs, pcms, col = [], [], 0
    for T, nb in calls:
        a, bl, rs = _call_rows(x, stereo, col, T, nb, s16)
        out, pcm, _ = _process(bank, a, bl, nb, rs, device)
        outs.append(out)
        pcms.append(pcm)
        col += T
    bank.close()
    return np.concatenate(outs, axis=1), np.concatenate(pcms, axis=1)


def test_call_split(gpu):
    """the same 400 frames in one call and cut three ways, with calls shorter than the history: bit for bit"""
    rng = np.random.default_rng(7)
    sessions = _sessions(70, rng)
    for k, p in enumerate(sessions.values()):
        p["bus"] = 2 if k % 17 == 3 else 0       # 66 in bus 0 (two chunks), 4 in bus 2, bus 1 empty
    x = rng.uniform(-0.2, 0.2, (70, 400, 2))
    stereo = _stereo_rows(sessions, 70)
    ref, rpcm = _run_split(sessions, x, stereo, [(400, 1)], 3)
    assert not _bits(ref[1]).any() and not rpcm[1].any() and np.abs(ref[0]).max() > 0.5 and np.abs(ref[2]).max() > 0
    for calls, device in (([(1, 1)] * 10 + [(390, 1)], False), ([(40, 2)] * 5 + [(200, 1)], True), ([(7, 1), (393, 3)], False)):
        out, pcm = _run_split(sessions, x, stereo, calls, 3, device)
        assert np.array_equal(_bits(out), _bits(ref)) and np.array_equal(pcm, rpcm), calls


def test_independence(gpu):
    """a bus's bits do not depend on the sessions of the other buses, on a NaN in another bus's input, or on a NaN carried by a
    muted session of its own"""
    rng = np.random.default_rng(8)
    sessions = _sessions(75, rng, nbuses=3)
    x = rng.uniform(-0.3, 0.3, (76, 90, 2))
    sessions[151] = dict(source=75, bus=0, channels=1, gain=1.0, pan=0.4, muted=1)
    stereo = _stereo_rows(sessions, 76)
    calls = [(60, 2), (30, 1)]
    ref, rpcm = _run_split(sessions, x, stereo, calls, 3)
    for b in range(3):
        alone = {s: p for s, p in sessions.items() if p["bus"] == b}
        out, pcm = _run_split(alone, x, stereo, calls, 3)
        assert np.array_equal(_bits(out[b]), _bits(ref[b])) and np.array_equal(pcm[b], rpcm[b]), b
    xn = x.copy()
    victim = next(p for p in sessions.values() if p["bus"] == 1 and not p.get("muted"))
    xn[victim["source"], 10] = np.nan
    xn[75, 3:50] = np.nan
    out, pcm = _run_split(sessions, xn, stereo, calls, 3)
    assert np.isnan(out[1]).any() and np.isfinite(out[0]).all()
    for b in (0, 2):
        assert np.array_equal(_bits(out[b]), _bits(ref[b])) and np.array_equal(pcm[b], rpcm[b]), b


def test_changes_mid_stream(gpu):
    """adjust, set, remove and a set over an occupied slot between calls of 20 frames (shorter than the history): the model's
    bound throughout; bus 1 holds one session, so there the kept and the zeroed history are read off directly"""
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.5, 0.5, (8, 160, 2))
    stereo = np.array([0, 1, 0, 0, 1, 0, 0, 0], bool)
    sessions = {0: dict(source=0, gain=0.5, pan=0.3), 1: dict(source=1, channels=2, gain=1.0, pan=-0.6),
                2: dict(source=2, gain=1.5, pan=0.0), 3: dict(source=3, gain=0.7, pan=-1.0),
                10: dict(source=6, bus=1, gain=1.0, pan=0.0)}
    bank, model = _both(RATE, 16, 2, 20, sessions)

    def both(f, *args, **kw):
        getattr(bank, f)(*args, **kw)
        getattr(model, f)(*args, **kw)

    steps = {1: lambda: (both("adjust", 0, 1.5, -0.8), both("adjust", 10, 1.0, 1.0)),          # new delays on the other side
             2: lambda: both("adjust", 1, 1.0, -0.6, 1),                                        # mute
             3: lambda: (both("adjust", 1, 0.9, 0.6, 0), both("set", 7, source=4, channels=2, gain=1.1, pan=0.9)),
             4: lambda: both("remove", 2),
             5: lambda: (both("set", 3, source=5, gain=1.2, pan=1.0), both("set", 10, source=7, bus=1, gain=1.0, pan=1.0)),
             6: lambda: both("set", 2, source=2, gain=0.4, pan=-1.0)}
    worst, outs = 0.0, []
    for c in range(8):
        steps.get(c, lambda: None)()
        a, bl, rs = _call_rows(x, stereo, 20 * c, 20, 1, False)
        out, pcm, st = _process(bank, a, bl, 1, rs, device=bool(c & 1))
        worst = _check(out, pcm, st, *model.process(a, bl, 1, rs), worst)
        outs.append(out)
    bank.close()
    # bus 1 after call 1: its one session sits at pan 1, gl = 0 and gr = 1 -- the left side all zero, the right the input
    assert np.array_equal(outs[1][1, :, 1], x[6, 20:40, 0].astype(np.float32))
    assert not outs[1][1, :, 0].any()
    print("mixer changes mid-stream: worst error %.3f of the bound" % worst)


def test_kept_and_zeroed_history(gpu):
    """one session alone in its bus, so the output is a single rounded product: after adjust the delayed side's first frames
    are the frames the session brought before; after a set over the occupied slot they are zero"""
    rng = np.random.default_rng(10)
    x = rng.uniform(-0.5, 0.5, (1, 90, 2))
    xf = x[0, :, 0].astype(np.float32)
    stereo = np.zeros(1, bool)
    bank = MonBank(RATE, 4, 1, 30)
    bank.set(2, source=0, gain=1.0, pan=0.0)
    outs = []
    for c in range(3):
        if c == 1:
            bank.adjust(2, 1.0, 0.5)      # gl = 0.25, dl = 24; gr = 0.75
        if c == 2:
            bank.set(2, source=0, gain=1.0, pan=0.5)
        a, bl, rs = _call_rows(x, stereo, 30 * c, 30, 1, False)
        outs.append(_process(bank, a, bl, 1, rs, device=False)[0][0])
    bank.close()
    assert mm.delays(0.5, RATE) == (24, 0)
    q, t = np.float32(0.25), np.float32(0.75)
    assert np.array_equal(outs[0][:, 0], np.float32(0.5) * xf[:30])
    assert np.array_equal(outs[1][:, 0], q * xf[30 - 24:60 - 24]) and np.array_equal(outs[1][:, 1], t * xf[30:60])
    assert not outs[2][:24, 0].any() and np.array_equal(outs[2][24:, 0], q * xf[60:66])
    assert np.array_equal(outs[2][:, 1], t * xf[60:90])


def test_a_receiver_banks_plane_in_place(gpu):
    """an FM, an AM and a stereo ISB channel of a small receiver bank mixed from its device audio plane on its stream, against
    the model run on the same audio pulled to the host"""
    FS, LB, MB, DRX, per_call = 12288000, 8192, 8193, 32, 4
    rx = kq.Bank(FS, LB, MB, DRX, 3, per_call)
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-8000.0, high=8000.0, second_lo=-1.0e6))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_AM_DEMOD, low=-5000.0, high=5000.0, second_lo=2.0e6))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=-5000.0, high=5000.0, second_lo=-3.0e6, hangtime=1.1,
                                     recovery_rate=6.0, isb=1, channels=2))
    olen, rate = rx.olen, FS // DRX
    mon = MonBank.beside(rx, max_sessions=4, max_buses=2)
    model = mm.MonModel(rate, 2)
    assert mon.samprate == rate == 384000 and mon.H == 384
    for slot, p in ((0, dict(source=0, gain=0.8, pan=0.5)), (1, dict(source=1, gain=1.0, pan=-1.0)),
                    (3, dict(source=2, channels=2, gain=0.6, pan=0.3))):
        mon.set(slot, **p)
        model.set(slot, **p)
    rng = np.random.default_rng(12)
    n = per_call * LB
    t = np.arange(3 * n) / FS
    sig = 3000 * np.exp(2j * np.pi * (1.0e6 * t + 2.0 * np.sin(2 * np.pi * 700 * t))) \
        + 3000 * (1 + 0.5 * np.sin(2 * np.pi * 500 * t)) * np.exp(-2j * np.pi * 2.0e6 * t) \
        + 2000 * np.exp(2j * np.pi * 3.0007e6 * t) + 1500 * np.exp(2j * np.pi * 2.9991e6 * t)
    worst = 0.0
    for c in range(3):
        s = sig[c * n:(c + 1) * n]
        iq = np.stack([s.real, s.imag], axis=1) + rng.normal(0, 100, (n, 2))
        rx.push_iq(np.clip(np.round(iq), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        T, out, pcm, st = mon.process_bank(rx)
        mon.sync()
        assert T == per_call * olen
        out, pcm, st = out.cpu().numpy(), pcm_array(pcm), status_array(st)
        plane = np.zeros((3, per_call, 2 * olen), np.float32)
        for ch in range(3):
            for b in range(per_call):
                a = rx.audio(ch, b)
                assert a.size == (2 * olen if ch == 2 else olen)
                plane[ch, b, :a.size] = a
        assert np.abs(plane).max() > 0
        worst = _check(out, pcm, st, *model.process(plane.reshape(3, -1), olen, per_call, 2 * olen), worst)
    mon.close()
    rx.close()
    print("mixer beside a receiver bank: worst error %.3f of the bound" % worst)


def test_another_rate_and_more_than_one_tile(gpu):
    """192 kHz (H = 192), one call of 1100 frames: two time tiles, two chunks"""
    rate, K, T = 192000, 65, 1100
    rng = np.random.default_rng(13)
    sessions = _sessions(K, rng)
    for p, pan in zip(sessions.values(), [-1.0, 1.0, 191.0 / 192, -191.0 / 192, 1.0 / 192, 0.0]):
        p["pan"] = pan
    assert [mm.delays(p["pan"], rate) for p in list(sessions.values())[:5]] == [(0, 192), (192, 0), (191, 0), (0, 191), (1, 0)]
    x = rng.uniform(-0.1, 0.1, (K, T, 2))
    stereo = _stereo_rows(sessions, K)
    bank, model = _both(rate, 2 * K + 2, 1, T, sessions)
    a, bl, rs = _call_rows(x, stereo, 0, T, 1, False)
    worst = 0.0
    for device in (True, False):      # the second call reads the first one's last 192 frames
        out, pcm, st = _process(bank, a, bl, 1, rs, device)
        worst = _check(out, pcm, st, *model.process(a, bl, 1, rs), worst)
    bank.close()
    print("mixer parity K %d at %d Hz, %d frames: worst error %.3f of the bound" % (K, rate, T, worst))
