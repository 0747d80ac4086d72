"""The float64 model of the monitor mixer (tests/mon_model.py) against an independent literal form: one shared stereo
output ring per bus, every session adding its packet at wptr + delay, as monitor.c:475-496 does; the delay rounding of
monitor.c:444-447; muted means absent."""
import numpy as np
import pytest

import mon_model as mm

RATE, H = 48000, 48


def literal(sessions, audio, calls, nbuses, fmt_s16):
    """sessions: slot -> (source, bus, channels, gain, pan, first_call).  A ring of 4096 frames per bus; per call and
    session the packet's samples are added at wptr + left_delay / wptr + right_delay (monitor.c:475-496), then the
    call's frames are read out and cleared, as the player's callback does.  Settings are constant per session, as they
    are within a packet."""
    size = 4096
    ring = np.zeros((nbuses, size, 2))
    outs, wptr, col = [], 0, 0
    for ci, T in enumerate(calls):
        for slot in sorted(sessions):
            source, bus, ch, gain, pan, first = sessions[slot]
            if ci < first:
                continue
            left_gain = np.float32(gain) * (np.float32(1) - np.float32(pan)) / np.float32(2)
            right_gain = np.float32(gain) * (np.float32(1) + np.float32(pan)) / np.float32(2)
            left_delay = right_delay = 0
            p = float(np.float32(pan))
            if p > 0:
                left_delay = int(np.floor(p * .001 * RATE + 0.5))
            elif p < 0:
                right_delay = int(np.floor(-p * .001 * RATE + 0.5))
            data = audio[source][col * ch:(col + T) * ch]
            left, right = wptr + left_delay, wptr + right_delay
            for i in range(T):
                if fmt_s16:
                    w = data[i * ch:(i + 1) * ch].view(">i2").astype(np.int16)
                    s = [float(mm.SCALE * np.float32(x)) for x in w]
                else:
                    s = [float(x) for x in data[i * ch:(i + 1) * ch]]
                ring[bus, left % size, 0] += s[0] * float(left_gain)
                ring[bus, right % size, 1] += s[-1] * float(right_gain)
                left += 1
                right += 1
        idx = np.arange(wptr, wptr + T) % size
        outs.append(ring[:, idx].copy())
        ring[:, idx] = 0
        wptr += T
        col += T
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("fmt_s16", [False, True])
def test_model_matches_literal_ring(fmt_s16):
    rng = np.random.default_rng(5)
    calls = [96, 5, 1, 130, 47, 48, 49]
    total = sum(calls)
    pans = [-1.0, 0.0, 1.0, 1.0 / H, -(H - 1.0) / H, 0.37, -0.61, 0.5]
    sessions = {}
    for k in range(40):
        sessions[3 * k + 1] = (k, k % 3, 1 + (k % 4 == 1), float(rng.uniform(0, 2)), pans[k % len(pans)] if k < 16 else
                               float(rng.uniform(-1, 1)), 0 if k % 5 else 2)
    x = rng.uniform(-1, 1, (40, 2 * total))
    audio = mm.to_s16be(x) if fmt_s16 else x.astype(np.float32)
    want = literal(sessions, audio, calls, 4, fmt_s16)
    # the model, call by call; a session's row holds its own frames back to back (2 values per frame if stereo), so its
    # call is cut out of the row and handed over as a row of its own
    model = mm.MonModel(RATE, 4)
    got, col = [], 0
    for ci, T in enumerate(calls):
        rows = np.zeros((40, 2 * T), audio.dtype)
        for slot, (source, bus, ch, gain, pan, first) in sessions.items():
            if ci == first:
                model.set(slot, source, bus, ch, gain, pan)
            rows[source, :ch * T] = audio[source, col * ch:(col + T) * ch]
        out, absum, nsess, active = model.process(rows, T)
        got.append(out)
        col += T
    got = np.concatenate(got, axis=1)
    assert np.all(got[3] == 0)                       # an empty bus
    assert np.abs(got[:3]).max() > 1.0
    assert np.abs(got - want).max() <= 1e-12


def test_delay_rounding():
    assert mm.history(RATE) == 48 and mm.history(192000) == 192 and mm.history(8000) == 8 and mm.history(44100) == 44
    assert mm.delays(0.0, RATE) == (0, 0)
    assert mm.delays(1.0, RATE) == (H, 0) and mm.delays(-1.0, RATE) == (0, H)
    # pan = 0.5 / H as a float: 0.010416667 (above 1 / 96), so the product is just above one half and rounds up
    p = np.float32(0.5 / H)
    assert float(p) * .001 * RATE > 0.5
    assert mm.delays(0.5 / H, RATE) == (1, 0) and mm.delays(-0.5 / H, RATE) == (0, 1)
    # ... and where the float falls below the half, down: H = 192, 0.5 / 192 = 0.0026041667 as a float is below 1 / 384
    q = np.float32(0.5 / 192)
    want = 1 if float(q) * .001 * 192000 >= 0.5 else 0
    assert mm.delays(0.5 / 192, 192000) == (want, 0) and mm.delays(-0.5 / 192, 192000) == (0, want)
    assert mm.delays(1.0 / H, RATE) == (1, 0) and mm.delays((H - 1.0) / H, RATE) == (H - 1, 0)
    assert mm.c_round(0.5) == 1 and mm.c_round(1.5) == 2 and mm.c_round(2.5) == 3 and mm.c_round(0.49999999999999994) == 0


def test_gains_are_float32():
    gl, gr = mm.gains(0.7, 0.3)
    assert gl.dtype == np.float32 and gr.dtype == np.float32
    assert gl == np.float32(0.7) * (np.float32(1) - np.float32(0.3)) / np.float32(2)
    assert mm.gains(1.0, 1.0) == (0.0, 1.0) and mm.gains(2.0, -1.0) == (2.0, 0.0) and mm.gains(1.0, 0.0) == (0.5, 0.5)


def test_muted_means_absent():
    rng = np.random.default_rng(6)
    audio = rng.uniform(-1, 1, (3, 64)).astype(np.float32)
    audio[1, 7] = np.nan
    a, b = mm.MonModel(RATE, 1), mm.MonModel(RATE, 1)
    for m in (a, b):
        m.set(0, source=0, gain=0.8, pan=-0.4)
        m.set(2, source=2, gain=1.3, pan=0.9)
    a.set(1, source=1, gain=1.0, pan=0.2, muted=1)
    oa, sa, ka, aa = a.process(audio, 64)
    ob, sb, kb, ab = b.process(audio, 64)
    assert np.array_equal(oa, ob) and np.array_equal(sa, sb) and np.all(np.isfinite(oa))
    assert ka[0] == kb[0] == 2 and aa[0] == ab[0] == 2
    # its input is still carried: unmuted, the delayed side starts in what it brought while muted
    audio2 = rng.uniform(-1, 1, (3, 64)).astype(np.float32)
    a.adjust(1, 1.0, 0.2, 0)
    o2, _, k2, _ = a.process(audio2, 64)
    assert k2[0] == 3 and np.isnan(o2[0, :, 1]).sum() == 0 and np.isnan(o2[0, :, 0]).sum() == 0   # frame 7 is 57 frames back, H = 48
    d = mm.delays(0.2, RATE)[0]
    b.set(1, source=1, gain=1.0, pan=0.2)
    o3, _, _, _ = b.process(audio2, 64)
    assert np.array_equal(o2[0, d:], o3[0, d:]) and not np.array_equal(o2[0, :d, 0], o3[0, :d, 0])


def test_scaleclip_and_pcm_words():
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -2.0, 0.99999994, -0.99999994, np.nan], np.float32)
    assert mm.scaleclip(x).tolist() == [0, 16383, -16383, 32767, -32768, 32767, -32768, 32766, -32766, 0]
    w = np.array([0x7fff, 0x8000, 0x0001, 0xffff], ">u2")
    f = mm.from_s16be(w)
    assert f.dtype == np.float32
    assert f.tolist() == [float(mm.SCALE * np.float32(v)) for v in (32767, -32768, 1, -1)]
