"""The spectrum bank (kq_spec_*, ka9q_sdr_amd/csrc/kq_spec.hip) on the GPU: against the float64 model of
tests/spec_model.py, bit for bit against itself under other call splits, other analyzers and reruns, under control
changes from this and another thread, on ModBank's synthesised stations, and beside a receiver bank on its stream."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.spectrum import KQ_IQ_CF32, SpecBank, spec_params
import spec_model as sm

pytestmark = pytest.mark.gpu


def _params(**kw):
    return spec_params(**kw), sm.params(**kw)


def _signal(rng, n, fs, tones, noise=0.01):
    """complex noise plus tones (frequency Hz, amplitude): every bin of a row within about 60 dB of its maximum"""
    t = np.arange(n)
    x = np.sqrt(noise / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, a in tones:
        x = x + a * np.exp(2j * np.pi * (f / fs * t + rng.uniform()))
    return x


def _as(x, fmt):
    if fmt == "cf32":
        return x.astype(np.complex64)
    scale = 32767 if fmt == "s16" else 127
    dt = np.int16 if fmt == "s16" else np.int8
    q = np.stack([x.real, x.imag], axis=1) * (0.25 * scale)
    return np.clip(np.round(q), -scale, scale).astype(dt)


def _check_rows(got, want):
    """each row's relative RMS <= 1e-5; every bin within 80 dB of the row's maximum within 0.01 dB"""
    assert got.shape == want.shape and len(want), (got.shape, want.shape)
    for g, w in zip(got.astype(np.float64), want):
        rr = np.sqrt(np.mean((g - w) ** 2) / np.mean(w ** 2))
        assert rr <= 1e-5, rr
        keep = w >= w.max() * 1e-8
        db = np.abs(10 * np.log10(g[keep] / w[keep]))
        assert db.max() <= 0.01, db.max()


def _feed(bank, iq, cuts, device):
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = iq[a:b]
        if device:
            t = torch.from_numpy(np.ascontiguousarray(part)).cuda()
            torch.cuda.synchronize()
            bank.process(t)
            bank.sync()
        else:
            bank.process(part)


PARITY = [
    # (fs, params, format, device, tones)
    (10000000, dict(fft_size=16384, hop=8192, average=2, center=1234567.0), "cf32", False, [(2e6, 0.3), (-3.3e6, 0.05)]),
    (10000000, dict(fft_size=15360, hop=5000, average=3, center=-2e6, kaiser_beta=4.0), "s16", True, [(-1.5e6, 0.3)]),
    (10000000, dict(decimate=8, fft_size=2048, hop=1024, average=2, center=3e5), "s8", False, [(3.1e5, 0.3), (2.0e5, 0.1)]),
    (10000000, dict(decimate=25, fft_size=4000, bins=3000, hop=2000, average=2, center=-1e6, sweep=2e6), "cf32", True,
     [(-1.02e6, 0.3)]),
    (2000000, dict(decimate=256, fft_size=256, hop=128, average=2, center=5e4), "s16", False, [(5.05e4, 0.2), (4.0e4, 0.2)]),
]


@pytest.mark.parametrize("fs,kw,fmt,device,tones", PARITY)
def test_parity_with_the_model(gpu, fs, kw, fmt, device, tones):
    p, mp = _params(**kw)
    Dz, Nf, H, K = p.decimate, p.fft_size, p.hop, p.average
    n = (24 * Dz if Dz > 1 else 0) + Dz * (Nf + 3 * K * H) + 777
    rng = np.random.default_rng(Dz * 100 + Nf)
    iq = _as(_signal(rng, n, fs, tones), fmt)
    gain = 0.8
    bank = SpecBank(fs, max_specs=4, max_samples=n // 2 + 1, max_rows=32, gain_factor=gain)
    bank.set(3, p)
    _feed(bank, iq, [0, n // 3, n // 2 + n // 3, n], device)
    rows, start, gen = bank.pull(3)
    info = bank.info(3)
    bank.close()
    want, wstart = sm.analyzer_rows(sm.convert(iq, gain), mp, fs)
    assert np.array_equal(start, wstart) and np.all(gen == 1)
    _check_rows(rows, want)
    mi = sm.info(mp, fs)
    for k in ("bin_bw", "first_bin_hz", "delay_samples"):
        assert info[k] == pytest.approx(mi[k], rel=1e-12)
    assert info["enbw_bins"] == pytest.approx(mi["enbw_bins"], rel=1e-6)
    assert info["rows_ready"] == 0 and info["generation"] == 1


SPLIT = [dict(decimate=8, fft_size=512, hop=100, average=3, center=1.2e5, sweep=-3e5),
         dict(fft_size=960, hop=500, average=2, center=-4e5),
         dict(decimate=25, fft_size=400, bins=300, hop=200, average=1, center=2.5e5)]


def _run(fs, plist, iq, cuts, max_samples, device=False, slots=None):
    bank = SpecBank(fs, max_specs=max(slots or [len(plist) - 1]) + 1, max_samples=max_samples, max_rows=4096)
    slots = slots or list(range(len(plist)))
    for s, kw in zip(slots, plist):
        bank.set(s, spec_params(**kw))
    _feed(bank, iq, cuts, device)
    out = [bank.pull(s) for s in slots]
    bank.close()
    return out


def test_same_bits_for_any_split(gpu):
    fs = 1000000
    n = 150000
    rng = np.random.default_rng(11)
    iq = _as(_signal(rng, n, fs, [(1.3e5, 0.3), (-4e5, 0.1)]), "s16")
    one = _run(fs, SPLIT, iq, [0, n], n)
    cuts = [0, 1, 2, 9, 16, 23, 99, 150, 151, 4000, 4001, 4007, 30000, 30050, 30051, 90000, n]   # 1-sample, < Dz, < H
    ragged = _run(fs, SPLIT, iq, cuts, 60000)
    dev = _run(fs, SPLIT, iq, [0, 5, 70000, n], 80000, device=True)
    for a, b, c in zip(one, ragged, dev):
        assert len(a[0]) > 5
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)


def test_analyzers_are_independent_and_reruns_repeat(gpu):
    fs = 1000000
    n = 120000
    rng = np.random.default_rng(5)
    iq = _as(_signal(rng, n, fs, [(1e5, 0.3), (-2.2e5, 0.2), (3.7e5, 0.05)]), "cf32")
    zooms = [(1, 256), (1, 1000), (4, 256), (8, 512), (25, 160), (64, 64)]
    plist = []
    for i in range(256):
        dz, nf = zooms[i % len(zooms)]
        plist.append(dict(decimate=dz, fft_size=nf, hop=nf // 2 if i % 3 else nf, average=1 + i % 3,
                          center=float(rng.uniform(-4.5e5, 4.5e5)), sweep=1e4 if i % 7 == 0 else 0.0))
    cuts = [0, 40000, 40001, n]
    together = _run(fs, plist, iq, cuts, 80000)
    again = _run(fs, plist, iq, cuts, 80000)
    for i, kw in enumerate(plist):
        alone = _run(fs, [kw], iq, cuts, 80000, slots=[i])[0]
        assert len(alone[0]) > 0
        for x, y, z in zip(together[i], again[i], alone):
            assert np.array_equal(x, y) and np.array_equal(x, z), i


def test_control_between_calls(gpu):
    fs = 1000000
    rng = np.random.default_rng(2)
    n = 200000
    iq = _as(_signal(rng, n, fs, [(1e5, 0.3), (-2e5, 0.1)]), "s16")
    bank = SpecBank(fs, max_specs=4, max_samples=50000, max_rows=5)
    model = sm.SpecModel(fs, max_rows=5)
    a = dict(decimate=4, fft_size=256, hop=128, average=2, center=1e5)
    b = dict(decimate=4, fft_size=256, hop=128, average=2, center=-2e5)            # same B: unpulled rows stay
    c = dict(fft_size=512, bins=400, hop=512, average=1, center=5e4)               # new B: unpulled rows are dropped
    steps = [("set", 0, a), ("set", 1, c), ("run", 30000), ("pull", 0), ("run", 17), ("set", 0, b), ("run", 40000),
             ("run", 3), ("pull", 1), ("set", 1, a), ("run", 50000), ("pull", 0), ("remove", 1), ("run", 20000),
             ("set", 1, c), ("run", 40000), ("pull", 0), ("pull", 1)]
    pos = 0
    for st in steps:
        if st[0] == "set":
            bank.set(st[1], spec_params(**st[2]))
            model.set(st[1], sm.params(**st[2]))
        elif st[0] == "remove":
            bank.remove(st[1])
            model.remove(st[1])
        elif st[0] == "run":
            bank.process(iq[pos:pos + st[1]])
            model.process(iq[pos:pos + st[1]])
            pos += st[1]
        else:
            s = st[1]
            info = bank.info(s)
            assert info["rows_ready"] == len(model.ready[s]) and info["rows_dropped"] == model.dropped[s], (st, info)
            rows, start, gen = bank.pull(s)
            wr, ws, wg = model.pull(s)
            assert np.array_equal(start, ws) and np.array_equal(gen, wg), (st, start, ws, gen, wg)
            _check_rows(rows, wr)
    assert model.dropped[0] > 0 and model.dropped[1] > 0
    bank.close()


def test_operator_thread_sets_while_processing(gpu):
    """an operator thread replaces the analyzer 12 times, each time after at least two more calls have been issued, while
    the main thread goes on processing and pulling; every row equals the model's row for the generation it names"""
    import time
    fs = 1000000
    rng = np.random.default_rng(9)
    n, chunk = 1000000, 5000
    iq = _as(_signal(rng, n, fs, [(1e5, 0.3), (-2e5, 0.1), (3e5, 0.2)]), "cf32")
    centers = [1e5, -2e5, 3e5, 0.0, -1e5, 2.5e5]

    def kw(g):   # the parameters of generation g
        return dict(decimate=4 if g % 2 else 8, fft_size=256, bins=192, hop=128, average=1, center=centers[g % len(centers)])

    bank = SpecBank(fs, max_specs=2, max_samples=chunk, max_rows=4096)
    bank.set(1, spec_params(**kw(1)))
    calls = [0]
    done, stop = threading.Event(), threading.Event()
    errors = []

    def operator():
        try:
            for g in range(2, 14):
                c = calls[0]
                while calls[0] < c + 2 and not stop.is_set():
                    time.sleep(0.0002)
                if stop.is_set():
                    break
                bank.set(1, spec_params(**kw(g)))
        except Exception as e:   # reported by the main thread
            errors.append(e)
        done.set()

    th = threading.Thread(target=operator)
    th.start()
    got = []
    pos, tail = 0, 3
    while pos + chunk <= n and tail:
        bank.process(iq[pos:pos + chunk])
        pos += chunk
        calls[0] += 1
        got.append(bank.pull(1))
        if done.is_set():
            tail -= 1          # a few more calls after the last change
    stop.set()
    th.join()
    got.append(bank.pull(1))
    bank.close()
    assert not errors, errors
    rows = np.concatenate([g[0] for g in got])
    start = np.concatenate([g[1] for g in got])
    gen = np.concatenate([g[2] for g in got])
    x = sm.convert(iq[:pos])
    assert len(np.unique(gen)) >= 10, np.unique(gen)
    for g in np.unique(gen):
        sel = gen == g
        s0 = int(start[sel].min())           # row 0 of a generation starts where it was set
        want, ws = sm.analyzer_rows(x, sm.params(**kw(int(g))), fs, s0=s0)
        m = int(sel.sum())
        assert np.array_equal(start[sel], ws[:m])
        _check_rows(rows[sel], want[:m])


def test_loopback_from_the_modulator_bank(gpu):
    """AM stations with carriers on bin centres at -10, -25 and -40 dBFS and a 1 kHz-ish tone: the overview reads each
    carrier at its level within 0.1 dB and nothing above -70 dBc where no station is; a zoom resolves one's sidebands"""
    from ka9q_sdr_amd.modulate import station_config
    fs, L, M, I = 192000, 4096, 4097, 4
    Nf = 16384
    bw = fs / Nf
    ks, levels = (-5120, -1707, 2560), (-10.0, -25.0, -40.0)
    zbw = fs / (16 * 1024)
    fa, depth = 85 * zbw, 0.3                     # audio tone on a zoom bin centre (996.1 Hz)
    mod = kq.ModBank(fs, L, M, I, max_stations=3, max_blocks=16)
    for s, (k, lv) in enumerate(zip(ks, levels)):
        mod.set_station(s, station_config("am", frequency=k * bw, amplitude_dbfs=lv))
    nblk = 16
    t = np.arange(4 * nblk * L // I) / (fs / I)
    audio = np.tile((depth * np.sin(2 * np.pi * fa * t)).astype(np.float32), (3, 1))
    spec = SpecBank(fs, max_specs=2, max_samples=nblk * L, max_rows=16)
    spec.set(0, spec_params(Nf, hop=Nf // 2, average=4))
    spec.set(1, spec_params(1024, decimate=16, hop=512, average=4, center=ks[0] * bw))
    La = nblk * L // I
    for c in range(4):
        out, _ = mod.process(audio[:, c * La:(c + 1) * La], nblk)
        spec.process(out)
    mod.close()
    wide, _, _ = spec.pull(0)
    zoom, _, _ = spec.pull(1)
    spec.close()
    assert len(wide) >= 2 and len(zoom) >= 2
    for row in wide[1:]:
        for k, lv in zip(ks, levels):
            assert abs(10 * np.log10(row[Nf // 2 + k]) - lv) < 0.1, (k, 10 * np.log10(row[Nf // 2 + k]), lv)
        empty = row[Nf // 2 + int(55000 / bw):Nf // 2 + int(85000 / bw)]
        assert 10 * np.log10(empty.max()) - levels[0] < -70
    B = 768
    for row in zoom[1:]:
        car = row[B // 2]
        assert abs(10 * np.log10(car) - levels[0]) < 0.1
        for sb in (B // 2 - 85, B // 2 + 85):
            side = 10 * np.log10(row[sb] / car)
            assert abs(side - 20 * np.log10(depth / 2)) < 0.2, side   # each sideband at depth / 2 of the carrier
            between = row[sb - 60:sb - 10] if sb > B // 2 else row[sb + 10:sb + 60]
            assert 10 * np.log10(between.max() / row[sb]) < -40          # resolved: deep valley beside it


def test_beside_a_receiver_bank_on_its_stream(gpu):
    from ka9q_sdr_amd import workload as wl
    from common import bank_cfg
    lib = kq.load_library()
    lib.kq_bank_stream.restype = C.c_void_p
    lib.kq_bank_stream.argtypes = [C.c_void_p]
    g = dict(samprate=192000, L=512, M=513, D=4)
    fs, L, M = g["samprate"], g["L"], g["M"]
    chans = wl.channel_plan("cfg1", 2)
    nblocks, nbatches = 8, 4
    iq = wl.make_iq(fs, nbatches * nblocks * L, seed=31).astype(np.complex64)
    hist = np.zeros(M - 1, np.complex64)
    wins = []
    for k in range(nbatches):
        batch = iq[k * nblocks * L:(k + 1) * nblocks * L]
        wins.append(torch.from_numpy(np.concatenate([hist, batch])).cuda())
        hist = batch[-(M - 1):]
    torch.cuda.synchronize()
    sp = spec_params(1024, hop=256, average=2, center=10000.0)
    sz = spec_params(512, decimate=8, hop=256, average=1, center=-20000.0)

    def run(with_bank, with_spec):
        bank = kq.Bank(fs, L, M, g["D"], len(chans), nblocks)
        for p in chans:
            bank.add_channel(bank_cfg(p))
        spec = SpecBank(fs, max_specs=2, max_samples=nblocks * L, max_rows=256, stream=lib.kq_bank_stream(bank.h))
        spec.set(0, sp)
        spec.set(1, sz)
        audio = [[] for _ in chans]
        for w in wins:
            if with_bank:
                assert bank.process_resident(w.data_ptr(), nblocks) == nblocks
            if with_spec:
                spec.process_device(w.data_ptr() + (M - 1) * 8, KQ_IQ_CF32, nblocks * L)
            if with_bank:
                bank.sync()
                for c in range(len(chans)):
                    audio[c] += [bank.audio(c, b) for b in range(nblocks)]
        spec.sync()
        rows = [spec.pull(s) for s in (0, 1)] if with_spec else None
        spec.close()
        bank.close()
        return audio, rows

    both_a, both_r = run(True, True)
    bank_a, _ = run(True, False)
    _, spec_r = run(False, True)
    for x, y in zip(both_a, bank_a):
        assert all(np.array_equal(a, b) for a, b in zip(x, y))
    for x, y in zip(both_r, spec_r):
        assert len(x[0]) > 0 and all(np.array_equal(a, b) for a, b in zip(x, y))
