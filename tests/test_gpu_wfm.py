"""The FM stereo decoder bank (kq_wfm_*, ka9q_sdr_amd/csrc/kq_wfm.hip) on the GPU: against the float64 model of
tests/wfm_model.py from host and device memory, bit for bit against itself under other call splits and other slots, a slot
set mid-stream, and a loopback from ModBank stations through a receiver bank's flat FM channels."""
import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.wfm import WfmBank, status_array, wfm_params
import wfm_model as wm

pytestmark = pytest.mark.gpu

FC, DA, L, M = 384000, 8, 2048, 2049     # Fo = 48 kHz, N = 4096
ON, OFF = 20.0, 14.0


def _composites(S, n, seed):
    """S composites: stereo tones, pilots from strong to absent, noise -- flags both on and off"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FC
    rows = []
    for s in range(S):
        lt = rng.uniform(0.1, 0.6) * np.sin(2 * np.pi * rng.uniform(200, 14000) * t)
        rt = rng.uniform(0.1, 0.6) * np.sin(2 * np.pi * rng.uniform(200, 14000) * t)
        pilot = [0.1, 0.1, 0.03, 0.0][s % 4]
        x = wm.multiplex(n, FC, lt, rt, pilot=pilot, pilot_hz=19000 + rng.uniform(-3, 3), phase=rng.uniform(0, 6))
        rows.append(x + 0.01 * rng.standard_normal(n))
    return np.array(rows)


def _run(bank, comp, calls, device=False):
    """comp [rows][n] in calls of (samples, nblocks); -> out [slots][j][2], status [slots][F]"""
    outs, sts = [], []
    pos = 0
    for n, nb in calls:
        chunk = np.ascontiguousarray(comp[:, pos:pos + n], np.float32)
        pos += n
        if not device:
            o, s = bank.process(chunk, nb)
        else:
            F = bank.frames(n)
            lo = F * L // DA
            dc = torch.from_numpy(chunk).cuda()
            do = torch.zeros((bank.max_slots, max(lo, 1), 2), dtype=torch.float32, device="cuda")
            ds = torch.zeros((bank.max_slots, max(F, 1), 4), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert bank.process_device(dc.data_ptr(), n, n // nb, n // nb, nb, do.data_ptr(), 2 * max(lo, 1), ds.data_ptr(),
                                       max(F, 1)) == F
            bank.sync()
            o, s = do[:, :lo].cpu().numpy(), status_array(ds[:, :F])
        outs.append(o)
        sts.append(s)
    return np.concatenate(outs, axis=1), np.concatenate(sts, axis=1)


def _check(out, st, want, wst):
    err = np.sqrt(np.mean((out - want) ** 2))      # relative to full scale 1.0
    assert err <= 2e-5, err
    near = (np.abs(wst["pilot_snr_db"] - ON) < 0.1) | (np.abs(wst["pilot_snr_db"] - OFF) < 0.1)
    flags_ok = (st["stereo"] == wst["stereo"]) | near
    # a frame after one whose flag may differ inherits the state: compare up to the first excused disagreement
    first = np.flatnonzero(~(st["stereo"] == wst["stereo"]))
    assert flags_ok.all() or (first.size and near[first[0]]), (st["stereo"], wst["stereo"])
    pil = wst["pilot_snr_db"] > 0
    assert np.all(np.abs(st["pilot_hz"][pil] - wst["pilot_hz"][pil]) <= 0.01), np.abs(st["pilot_hz"] - wst["pilot_hz"])[pil].max()
    return err


@pytest.mark.parametrize("S,deemph,device", [(1, 75.0, False), (3, 50.0, True), (3, 0.0, False), (64, 75.0, True)])
def test_parity_with_the_model(gpu, S, deemph, device):
    n = 12 * L
    comp = _composites(S, n, seed=S)
    src = [(7 * s) % S for s in range(S)]       # slot s decodes row src[s]
    bank = WfmBank(FC, DA, L, M, max_slots=S, max_samples=4 * L)
    model = wm.WfmModel(FC, DA, L, M)
    for s in range(S):
        bank.set(s, wfm_params(source=src[s], deemph_us=deemph, pilot_on_db=ON, pilot_off_db=OFF))
    out, st = _run(bank, comp, [(4 * L, 4)] * 3, device)
    bank.close()
    worst = 0.0
    seen = set()
    for s in range(S):
        want, wst = model.decode(comp[src[s]].astype(np.float32), deemph_us=deemph, pilot_on_db=ON, pilot_off_db=OFF)
        worst = max(worst, _check(out[s], st[s], want, wst))
        seen.update(wst["stereo"].tolist())
    print("wfm parity S=%d deemph=%g device=%d: worst relative RMS %.2e" % (S, deemph, device, worst))
    assert seen == {0, 1}


def test_split_and_independence(gpu):
    S, n = 3, 10 * L
    comp = _composites(S, n, seed=5)
    ref = WfmBank(FC, DA, L, M, max_slots=S, max_samples=n)
    for s in range(S):
        ref.set(s, wfm_params(source=s))
    want, wst = _run(ref, comp, [(n, 1)])
    ref.close()
    for calls in ([(1000, 1), (3000, 3), (2480, 2), (8000, 5), (6000, 4)], [(L, 1)] * 10, [(7 * 512, 7), (13 * 500, 13),
                                                                                          (n - 7 * 512 - 13 * 500, 1)]):
        b = WfmBank(FC, DA, L, M, max_slots=S, max_samples=n)
        for s in range(S):
            b.set(s, wfm_params(source=s))
        got, gst = _run(b, comp, calls, device=calls[0][0] == L)
        b.close()
        assert np.array_equal(got, want), calls
        assert np.array_equal(gst, wst), calls
    # each slot alone (in another slot number) gives the bits it gave beside the others
    for s in range(S):
        b = WfmBank(FC, DA, L, M, max_slots=4, max_samples=n)
        b.set(3, wfm_params(source=s))
        got, gst = _run(b, comp, [(n, 2)])
        b.close()
        assert np.array_equal(got[3], want[s]) and np.array_equal(gst[3], wst[s]), s


def test_parity_at_an_odd_decimated_size(gpu):
    """N = 5000, N / Da = 625 = 5^4: the decimated inverse transform runs the mixed-radix path at an odd size"""
    Lg, Mg = 3000, 2001
    n = 8 * Lg
    comp = _composites(1, n, seed=21)
    bank = WfmBank(FC, DA, Lg, Mg, max_slots=1, max_samples=4 * Lg)
    bank.set(0, wfm_params(deemph_us=75.0, pilot_on_db=ON, pilot_off_db=OFF))
    out, st = _run(bank, comp, [(4 * Lg, 4)] * 2)
    bank.close()
    want, wst = wm.WfmModel(FC, DA, Lg, Mg).decode(comp[0].astype(np.float32), deemph_us=75.0, pilot_on_db=ON,
                                                   pilot_off_db=OFF)
    print("wfm parity at N / Da = 625: relative RMS %.2e" % _check(out[0], st[0], want, wst))


def test_slot_set_mid_stream(gpu):
    n = 10 * L
    comp = _composites(2, n, seed=9)
    b = WfmBank(FC, DA, L, M, max_slots=2, max_samples=4 * L)
    b.set(0, wfm_params(source=0))
    first = 3 * L + 700                        # not on a frame boundary
    chunk = np.ascontiguousarray(comp[:, :first], np.float32)
    F = b.frames(first)
    o1 = np.full((2, F * L // DA, 2), np.nan, np.float32)
    assert b.lib.kq_wfm_process(b.h, chunk.ctypes.data, first, first, first, 1, 0, o1.ctypes.data, 2 * o1.shape[1], None, 0) == F
    b.n += first
    assert np.isfinite(o1[0]).all() and np.isnan(o1[1]).all()   # nothing written for the slot before it was set
    b.set(1, wfm_params(source=1))             # cold start at stream index `first`
    o2, s2 = _run(b, comp[:, first:], [(3 * L, 3), (n - first - 3 * L, 1)])
    b.close()
    x = comp[1].astype(np.float32).astype(np.float64)
    x[:first] = 0.0
    want, wst = wm.WfmModel(FC, DA, L, M).decode(x)
    F0 = first // L
    j0 = F0 * L // DA
    _check(o2[1], s2[1], want[j0:], {k: v[F0:] for k, v in wst.items()})


# ---- loopback: ModBank -> receiver Bank (flat FM) -> WfmBank.process_bank on the bank's stream ------------------------
FS, INTERP, LB, MB, DRX = 12288000, 32, 8192, 8193, 32
# Channel filter +-150 kHz and 75 kHz deviation: the same loopback through float64 (ideal FM synthesis, brick-wall channel
# filter, discriminator, tests/wfm_model.py) measured 41.8 dB of separation at 1 kHz (L) and 2.5 kHz (R) -- the model's
# figure, with the receiver noise below.  The GPU chain is held to 30 dB.
CH_BW, DEV, SEP_DB = 150000.0, 75000.0, 30.0


@pytest.mark.parametrize("overlap", [False, True])
def test_loopback_through_the_receiver(gpu, overlap):
    """overlap: an AM channel beside the FM ones makes the bank run each call's demodulators on its second stream, beside
    its next call; the decode in place must still read the finished plane: bit for bit what a second decoder makes of
    the same plane pulled to the host"""
    per_call, calls = 16, 12
    La = LB // INTERP
    n = per_call * calls * La
    rate = FS / INTERP
    t = np.arange(n) / rate
    stations = [(-2.0e6, "L", 1000.0), (1.0e6, "R", 2500.0), (3.5e6, "mono", 1500.0)]
    pcm = np.zeros((3, n), np.float32)
    for s, (_, side, hz) in enumerate(stations):
        tone = 0.9 * np.sin(2 * np.pi * hz * t)
        if side == "mono":
            pcm[s] = 0.9 * tone       # no pilot, no subcarrier
        else:
            m = wm.multiplex(n, rate, tone if side == "L" else 0.0, tone if side == "R" else 0.0, deviation_hz=DEV)
            pcm[s] = m * rate / (2 * np.pi * DEV)   # the multiplex in units of full deviation
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=3, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 4, per_call)
    for s, (f, _, _) in enumerate(stations):
        mod.set_station(s, kq.station_config("fm", frequency=f, amplitude_dbfs=-20.0, deviation=DEV, low=-60000.0, high=60000.0))
        rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-CH_BW, high=CH_BW, second_lo=-f, flat=1))
    if overlap:
        rx.add_channel(kq.channel_config(demod_type=kq.KQ_AM_DEMOD, low=-5000.0, high=5000.0, second_lo=5.0e6))
    wfm = WfmBank.beside(rx, DA, L, M, max_slots=3)
    twin = WfmBank(int(rate), DA, L, M, max_slots=3, max_samples=per_call * rx.olen)
    for s in range(3):
        wfm.set(s, wfm_params(source=s, deviation_hz=DEV, deemph_us=0.0))
        twin.set(s, wfm_params(source=s, deviation_hz=DEV, deemph_us=0.0))
    rng = np.random.default_rng(11)
    outs, sts = [], []
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)   # receiver noise (see test_gpu_modulate)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        F, o, st = wfm.process_bank(rx)
        o, st = o.cpu().numpy(), status_array(st)     # ordered after the decode on torch's stream
        plane = np.array([np.concatenate([rx.audio(s, b) for b in range(per_call)]) for s in range(3)])
        to, tst = twin.process(plane)
        assert np.array_equal(o, to) and np.array_equal(st, tst), c
        outs.append(o)
        sts.append(st)
    out, st = np.concatenate(outs, axis=1), np.concatenate(sts, axis=1)
    mod.close()
    rx.close()
    wfm.close()
    twin.close()
    skip = out.shape[1] // 4
    for s, (_, side, hz) in enumerate(stations):
        y = out[s, skip:]
        amp = [wm.tone_amp(y[:, c], FC / DA, hz) for c in (0, 1)]
        if side == "mono":
            assert not st[s]["stereo"].any()
            assert np.array_equal(out[s, :, 0], out[s, :, 1])
            print("loopback mono: L = R, flag 0, tone %.3f" % amp[0])
            continue
        assert st[s]["stereo"][2:].all(), st[s]["stereo"]
        want, leak = (amp[0], amp[1]) if side == "L" else (amp[1], amp[0])
        sep = 20 * np.log10(want / leak)
        print("loopback %s (overlap %d): tone %.3f, separation %.1f dB, pilot %.2f Hz" % (
            side, overlap, want, sep, np.median(st[s]["pilot_hz"][2:])))
        assert want > 0.8 and sep >= SEP_DB


def test_shared_rows_and_gaps_from_host_equal_device(gpu):
    """Slots {0, 1, 3, 6} of 8 on source rows {2, 0, 2, 1}: two slots share a row, the active list has gaps, and the blocks
    lie in rows wider than a block.  Two host-memory calls (distinct rows staged, planes copied back a run of slots at a
    time) give bit for bit what a twin bank gives from device memory, and leave everything else of the host buffers alone."""
    S, slots, nb, bl, pad = 8, {0: 2, 1: 0, 3: 2, 6: 1}, 3, 1500, 200
    n = nb * bl
    comp = _composites(3, 2 * n, seed=31).astype(np.float32)
    host, twin = (WfmBank(FC, DA, L, M, max_slots=S, max_samples=n) for _ in range(2))
    for b in (host, twin):
        for s, src in slots.items():
            b.set(s, wfm_params(source=src))
    for c in range(2):
        buf = np.full((3, nb, bl + pad), np.nan, np.float32)
        buf[:, :, :bl] = comp[:, c * n:(c + 1) * n].reshape(3, nb, bl)
        F = host.frames(n)
        ow, sw = 4 * 2 * (F * L // DA), 16 * F               # bytes of a slot's row that the call writes
        assert F >= 2
        out, st = np.full((S, ow + 24), 0xFF, np.uint8), np.full((S, sw + 16), 0xFF, np.uint8)
        assert host.lib.kq_wfm_process(host.h, buf.ctypes.data, nb * (bl + pad), bl + pad, bl, nb, 0, out.ctypes.data,
                                       out.shape[1] // 4, st.ctypes.data, st.shape[1] // 16) == F
        host.n += n
        dbuf = torch.from_numpy(buf).cuda()
        dout, dst = torch.from_numpy(np.full_like(out, 0xFF)).cuda(), torch.from_numpy(np.full_like(st, 0xFF)).cuda()
        torch.cuda.synchronize()
        assert twin.process_device(dbuf.data_ptr(), nb * (bl + pad), bl + pad, bl, nb, dout.data_ptr(), out.shape[1] // 4,
                                   dst.data_ptr(), st.shape[1] // 16) == F
        twin.sync()
        dout, dst = dout.cpu().numpy(), dst.cpu().numpy()
        for s in range(S):
            if s in slots:
                assert np.array_equal(out[s, :ow], dout[s, :ow]) and np.array_equal(st[s, :sw], dst[s, :sw]), (c, s)
                audio = out[s, :ow].view(np.float32)
                assert np.isfinite(audio).all() and audio.any(), (c, s)
                assert (out[s, ow:] == 0xFF).all() and (st[s, sw:] == 0xFF).all(), (c, s)
            else:
                assert (out[s] == 0xFF).all() and (st[s] == 0xFF).all(), (c, s)
        # the slots that share row 2 decode the same samples
        assert np.array_equal(out[0, :ow], out[3, :ow]) and not np.array_equal(out[0, :ow], out[1, :ow])
    host.close()
    twin.close()
