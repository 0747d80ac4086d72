"""The FSK / GMSK packet decoder bank (kq_fsk_*, ka9q_sdr_amd/csrc/kq_fsk.hip) on the GPU against the integer model of
tests/fsk_model.py: frame records (bytes, end_sample, end_bit), arena counts and every status field equal, bit for bit, with
no tolerance anywhere -- from host and device memory, float and big-endian int16 input, under other call splits, beside
other slots, set mid-stream, removed, reset, with a full arena, with bad and aborted frames, and in a loopback from two
ModBank stations through a receiver bank's flat FM channels.  The model runs on the bank's own taps (kq_fsk_get_taps;
tests/test_fsk_args.py holds them within one LSB of the model's design), so nothing in the comparison is floating point
but the quantiser's one multiply."""
import functools

import numpy as np
import pytest
import torch

import bank_gpu
import ka9q_sdr_amd as kq
import fsk_model as fm
from ka9q_sdr_amd.fsk import STATUS_DTYPE, TILE, FskBank, fsk_params, status_array
from test_fsk_model import sent

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _row(Fs, baud, s, count=2, amp=None):
    """slot s's burst: G3RUH on even slots, AIS on odd ones; clock error 0 / +-100 ppm; amplitude 0.3, 0.05 or 1 rad/sample,
    DC up to half of it, noise up to a tenth of it"""
    rng = np.random.default_rng(100 + s)
    scrambled = s % 2 == 0
    frames = fm.make_frames(count, 300 + s % 7, lo=12, hi=24)
    amp = amp or (0.3, 0.05, 1.0)[s % 3]
    x = fm.fsk_signal(frames, Fs, baud, scrambled, (0.0, 100.0, -100.0)[s % 3], amp, amp * rng.uniform(-0.5, 0.5),
                      amp * (0.0, 0.03, 0.1)[(s // 2) % 3], seed=s, lead=(10 + s % 5) / baud, tail=24.0 / baud,
                      preamble=not scrambled, lead_flags=8 if scrambled else 2)
    x.setflags(write=False)
    return frames, x


def _rows(Fs, baud, S, **kw):
    rows = [_row(Fs, baud, s, **kw) for s in range(S)]
    n = max(len(x) for _, x in rows)
    return [f for f, _ in rows], np.array([np.concatenate([x, np.full(n - len(x), x[-1], np.float32)]) for _, x in rows])


def _models(bank, S, **kw):
    hq = bank.get_taps()
    return [fm.FskModel(bank.samprate, bank.baud, bank.taps, scrambled=s % 2 == 0, taps=hq, max_frame_bytes=bank.max_frame_bytes,
                        **kw) for s in range(S)]


def _setup(bank, S):
    for s in range(S):
        bank.set(s, fsk_params(source=s, scrambled=s % 2 == 0))


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "frames"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "frame")
_device_call = functools.partial(bank_gpu.device_call, status_array)


# Fs, baud, K, window_bits, slots: 5, 4.07 and 40 samples per bit; K = 3 and 127; W = 2 and 1024; 65 slots put k_fsk_track on two
# waves.  (With K = 3 or W = 2 little decodes; the bits still have to be the model's.)
PARITY = [(48000, 9600, 21, 16.0, 1), (39062, 9600, 17, 16.0, 3), (384000, 9600, 127, 25.6, 3), (48000, 9600, 3, 0.4, 3),
          (48000, 9600, 127, 16.0, 2), (48000, 9600, 21, 16.0, 65)]


@pytest.mark.parametrize("Fs,baud,K,wb,S", PARITY)
def test_parity_from_host_and_device_memory(gpu, Fs, baud, K, wb, S):
    frames, x = _rows(Fs, baud, S)
    n = x.shape[1]
    cap = n // 3 + 64
    cuts = _chunks(n, (cap, 257, n // 4))                    # several calls, none on a word boundary but the first
    decoded = 0
    for device in (False, True):
        bank = FskBank(Fs, baud, K, S, cap, window_bits=wb)
        assert bank.get_taps().sum() in range(32768 - K, 32768 + K)
        _setup(bank, S)
        models = _models(bank, S, window_bits=wb)
        st_t = torch.zeros((S, 8), dtype=torch.int32, device="cuda")
        for a, b in cuts:
            nblocks = 4 if (b - a) % 4 == 0 else 1
            if device:
                st = _device_call(bank, x[:, a:b], nblocks, st_t)
            else:
                st = bank.process(x[:, a:b], nblocks)
            for s, m in enumerate(models):
                m.feed(x[s, a:b])
            _check(bank, _snap(models), st, what=(device, a, b))
        decoded = sum([f[0] for f in m.frames] == sent(frames[s]) for s, m in enumerate(models))
        bank.close()
    print("fsk parity %s: %d of %d slots decode every frame" % ((Fs, baud, K, wb, S), decoded, S))
    if K >= 17 and wb >= 16.0:
        assert decoded == S


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal far beyond the quantiser's range"""
    Fs, baud, K, S = 48000, 9600, 21, 2
    frames, x = _rows(Fs, baud, S, amp=20.0)                # 20 rad/sample x 4096: clips at +-32767
    assert (np.abs(x) * 4096 > 40000).mean() > 0.3
    words = fm.quantise(x * np.float32(0.02), 4096.0).astype(np.int16)
    words[:, 5:40:7] = -32768
    words[0, -3:] = -32768
    st_t = torch.zeros((S, 8), dtype=torch.int32, device="cuda")
    for data, fmt in ((x, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = FskBank(Fs, baud, K, S, 4096)
        _setup(bank, S)
        models = _models(bank, S)
        for a, b in _chunks(x.shape[1], (1000, 2048)):
            st = _device_call(bank, data[:, a:b], 1, st_t, fmt) if device else bank.process(data[:, a:b], 1, fmt)
            for s, m in enumerate(models):
                m.feed(data[s, a:b], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, a, b))
        assert all([f[0] for f in m.frames] == sent(frames[s]) for s, m in enumerate(models))
        bank.close()


SPLITS = [(1,), (63,), (64,), (65,), (TILE - 1,), (TILE,), (TILE + 1,), (2 * TILE + 64,), (7, 1100, 64, 129)]


def test_call_splits_change_nothing(gpu):
    """the same stream in calls of 1, 63, 64, 65, tile - 1, tile, tile + 1 and max_samples samples, in one block or many:
    identical records (end_sample included), counts and status, those of the model fed in one piece"""
    Fs, baud, K, S = 39062, 9600, 17, 2
    frames, x = _rows(Fs, baud, S, count=4)
    cap = 2 * TILE + 64
    assert x.shape[1] > cap + TILE
    ref = None
    for sizes in SPLITS:
        bank = FskBank(Fs, baud, K, S, cap)
        _setup(bank, S)
        if ref is None:
            ref = _models(bank, S)
            for s, m in enumerate(ref):
                m.feed(x[s])
            assert [len(m.frames) for m in ref] == [4, 4]
        for a, b in _chunks(x.shape[1], sizes):
            n = b - a
            nblocks = next(k for k in (8, 3, 2, 1) if n % k == 0)
            st = bank.process(x[:, a:b], nblocks)
        _check(bank, _snap(ref), st, what=sizes)
        bank.close()


def test_slot_beside_others_and_set_midstream(gpu):
    """a slot gives beside 64 others what it gives alone; a slot set after the first call sees zeros before its set and
    counts end_sample on the shared grid"""
    Fs, baud, K, S = 48000, 9600, 21, 65
    frames, x = _rows(Fs, baud, S)
    first = 50                                               # inside a word, before slot 9's burst begins
    big = FskBank(Fs, baud, K, S, 4096)
    for s in range(S):
        if s != 9:
            big.set(s, fsk_params(source=s, scrambled=s % 2 == 0))
    alone = FskBank(Fs, baud, K, 1, 4096)
    alone.set(0, fsk_params(source=7, scrambled=False))
    late = fm.FskModel(Fs, baud, K, scrambled=False, taps=big.get_taps(), start=first)
    for a, b in ((0, first), (first, x.shape[1])):
        st = big.process(x[:, a:b])
        sa = alone.process(x[:8, a:b])
        if a == 0:
            assert not st[9].tobytes().strip(b"\0")
            big.set(9, fsk_params(source=9, scrambled=False))
        else:
            late.feed(x[9, a:b])
    assert _status(st[7]) == _status(sa[0]) and big.frames(7) == alone.frames(0) and [f[0] for f in alone.frames(0)] == sent(frames[7])
    assert _status(st[9]) == late.status() and big.frames(9) == late.frames and len(late.frames) == 2
    assert late.frames[0][1] > first
    big.close()
    alone.close()


def test_remove_reset_full_arena_and_clear(gpu):
    Fs, baud, K = 48000, 9600, 21
    frames, x = _rows(Fs, baud, 2, count=4)
    bank = FskBank(Fs, baud, K, 2, 8192, max_frames=2)
    assert x.shape[1] <= 8192
    _setup(bank, 2)
    models = _models(bank, 2, max_frames=2)
    st = bank.process(x)
    for s, m in enumerate(models):
        m.feed(x[s])
    _check(bank, _snap(models), st)
    # the arena holds two: the first two stay intact, the others are counted
    assert [int(st[s]["dropped"]) for s in range(2)] == [2, 2] and [int(st[s]["frames_good"]) for s in range(2)] == [4, 4]
    assert [f[0] for f in bank.frames(1)] == sent(frames[1])[:2]
    # clear_frames empties the arenas and nothing else
    bank.clear_frames()
    assert not bank.counts().any()
    for m in models:
        m.clear_frames()
    st = bank.process(x)
    for s, m in enumerate(models):
        m.feed(x[s])
    _check(bank, _snap(models), st)
    assert [int(st[s]["dropped"]) for s in range(2)] == [4, 4] and list(bank.counts()) == [2, 2]
    assert bank.frames(0)[0][1] > x.shape[1]                  # end_sample runs on
    # a removed slot stops: nothing is written for it, its arena stays; the other goes on
    bank.remove(0)
    bank.clear_frames()
    models[1].clear_frames()
    st = bank.process(x)
    models[1].feed(x[1])
    assert not st[0].tobytes().strip(b"\0")
    _check(bank, _snap(models), st, slots=[1])
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, 2, max_frames=2)
    st = bank.process(x)
    fresh[1].feed(x[1])
    _check(bank, _snap(fresh), st, slots=[1])
    assert bank.frames(1)[0][1] < x.shape[1] and int(bank.counts()[0]) == 0
    bank.close()


def test_bad_and_aborted_frames(gpu):
    """a frame with one flipped bit and one longer than max_frame_bytes land in frames_bad; seven ones inside a frame count
    in aborts"""
    Fs, baud, K = 48000, 9600, 21
    rng = np.random.default_rng(21)
    frames = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (20, 30, 20)]
    bits = fm.afsk_bits(frames)
    flip = list(bits)
    flip[8 * 8 + 41] ^= 1
    abort = bits[:8 * 8 + 60] + [1] * 9 + bits[8 * 8 + 60:]
    sig = [np.concatenate([np.zeros(100), 0.3 * fm.shape(fm.line_bits(b, False), Fs, baud), np.zeros(200)]) for b in (bits, flip, abort)]
    n = max(len(v) for v in sig)
    x = np.array([np.concatenate([v, np.zeros(n - len(v))]) for v in sig], np.float32)
    for mfb, want in ((512, [(3, 0, 1), (2, 1, 1), (2, 0, 2)]), (24, [(2, 1, 1), (1, 2, 1), (1, 1, 2)])):
        bank = FskBank(Fs, baud, K, 3, x.shape[1], max_frame_bytes=mfb)
        hq = bank.get_taps()
        models = [fm.FskModel(Fs, baud, K, scrambled=False, taps=hq, max_frame_bytes=mfb) for _ in range(3)]
        for s in range(3):
            bank.set(s, fsk_params(source=s, scrambled=0))
        st = bank.process(x)
        for s, m in enumerate(models):
            m.feed(x[s])
        _check(bank, _snap(models), st, what=mfb)
        got = [(int(r["frames_good"]), int(r["frames_bad"]), int(r["aborts"])) for r in st[:3]]
        assert got == want, (mfb, got)
        bank.close()


# ---- loopback: two FM stations through a receiver bank, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """A G3RUH stream and an AIS burst, each on an FM station of 3 kHz deviation whose audio band passes DC to 7 kHz; a
    receiver bank with two flat FM channels at 48 kHz.  The decode in place on the bank's stream must read the finished
    plane: bit for bit what a twin bank makes of the same plane pulled to the host, and every frame sent comes out, in order."""
    per_call, baud, K = 64, 9600, 21
    rate = FS // INTERP
    La = LB // INTERP
    sent_frames = [fm.make_frames(4, 41), fm.make_frames(2, 42, lo=18, hi=22)]
    pcm = [fm.fsk_signal(sent_frames[0], rate, baud, True, amp=1.0, lead=0.02, tail=0.02),
           fm.fsk_signal(sent_frames[1], rate, baud, False, amp=1.0, lead=0.03, tail=0.02, preamble=True, lead_flags=2)]
    calls = max(len(p) for p in pcm) // (per_call * La) + 2
    n = calls * per_call * La
    pcm = np.array([np.concatenate([p, np.zeros(n - len(p), np.float32)]) for p in pcm])
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=2, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 2, per_call)
    assert rx.olen == La
    for s, f in enumerate((1.0e6, -1.5e6)):
        mod.set_station(s, kq.station_config("fm", frequency=f, amplitude_dbfs=-20.0, deviation=3000.0, low=-7000.0, high=7000.0))
        rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-10000.0, high=10000.0, second_lo=-f, flat=1))
    fsk = FskBank.beside(rx, baud, K, max_slots=2)
    twin = FskBank(rate, baud, K, 2, per_call * rx.olen)
    for b in (fsk, twin):
        b.set(0, fsk_params(source=0, scrambled=1))
        b.set(1, fsk_params(source=1, scrambled=0))
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)   # receiver noise (see test_gpu_modulate)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(fsk.process_bank(rx))                             # ordered after the decode
        plane = np.array([np.concatenate([rx.audio(ch, b) for b in range(per_call)]) for ch in range(2)])
        tst = twin.process(plane)
        assert np.array_equal(st, tst), (c, st, tst)
        assert np.array_equal(fsk.counts(), twin.counts())
    print("fsk loopback:", [_status(r) for r in st])
    for s in range(2):
        got = fsk.frames(s)
        assert got == twin.frames(s)
        assert [f[0] for f in got] == sent(sent_frames[s]), (s, len(got), _status(st[s]))
    for h in (mod, rx, fsk, twin):
        h.close()


@pytest.mark.parametrize("fmt", [kq.KQ_PCM_F32, kq.KQ_PCM_S16BE])
def test_shared_rows_and_gaps_from_host_equal_device(gpu, fmt):
    """Slots {0, 1, 3, 6} of 8 on source rows {2, 0, 2, 1}: two slots share a row, the active list has gaps, and the blocks
    lie in rows wider than a block.  Two host-memory calls (distinct rows staged, status copied back a run of slots at a
    time) give bit for bit what a twin bank gives from device memory, and leave everything else of the host buffer alone."""
    Fs, baud, K, wb = 48000, 9600, 21, 16.0
    S, slots, nb, pad = 8, {0: 2, 1: 0, 3: 2, 6: 1}, 3, 5
    frames, x = _rows(Fs, baud, 3)
    bl = x.shape[1] // (2 * nb)
    n = nb * bl
    if fmt == kq.KQ_PCM_S16BE:
        x = fm.quantise(x, 4096.0).astype(">i2").view(np.int16)
        junk = 0x0080
    else:
        junk = np.nan
    host, twin = (FskBank(Fs, baud, K, S, n, window_bits=wb) for _ in range(2))
    for b in (host, twin):
        for s, src in slots.items():
            b.set(s, fsk_params(source=src, scrambled=src % 2 == 0))
    sw = STATUS_DTYPE.itemsize
    for c in range(2):
        buf = np.full((3, nb, bl + pad), junk, x.dtype)
        buf[:, :, :bl] = x[:, c * n:(c + 1) * n].reshape(3, nb, bl)
        st = np.full((S, 2 * sw), 0xFF, np.uint8)            # status_stride 2: every second record is not the bank's
        assert host.lib.kq_fsk_process(host.h, buf.ctypes.data, fmt, nb * (bl + pad), bl + pad, bl, nb, 0, st.ctypes.data, 2) == 0
        host.n += n
        dbuf = torch.from_numpy(buf).cuda()
        dst = torch.from_numpy(np.full_like(st, 0xFF)).cuda()
        torch.cuda.synchronize()
        twin.process_device(dbuf.data_ptr(), nb * (bl + pad), bl + pad, bl, nb, dst.data_ptr(), 2, fmt=fmt)
        twin.sync()
        dst = dst.cpu().numpy()
        hc, tc = host.counts(), twin.counts()
        for s in range(S):
            if s in slots:
                assert np.array_equal(st[s, :sw], dst[s, :sw]) and (st[s, sw:] == 0xFF).all(), (c, s)
                assert hc[s] == tc[s] and host.frames(s, int(hc[s])) == twin.frames(s, int(tc[s])), (c, s)
            else:
                assert (st[s] == 0xFF).all() and hc[s] == 0, (c, s)
    # every frame sent is there, twice for the shared row
    for s in slots:
        assert [f[0] for f in host.frames(s)] == sent(frames[slots[s]]), s
    assert host.frames(0) == host.frames(3)
    host.close()
    twin.close()
