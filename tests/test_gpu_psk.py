"""The PSK decoder bank (kq_psk_*, ka9q_sdr_amd/csrc/kq_psk.hip) on the GPU against the integer model of
tests/psk_model.py: events (code, flags, end_sample, sig, rot_r, rot_i), arena counts and every field of the status record
-- the counters, the clock, the early, centre and late powers, both symbols' window sums, the rotation estimate, the levels,
the shift register, the last window sums and the open frame's I and Q -- equal after every call, with no tolerance
anywhere.  From host and device memory, float and big-endian int16 input, padded rows, slots that share a row at pitches
50 Hz apart, calls of 1, 23, 24, 25, 80, 4096 and 9000 samples (the last is six pieces of 64 frames to a wave at B = 24), on
70 slots (18 workgroups of k_psk, the last half empty) with two baud rates side by side (W = 16 and 8 within a workgroup),
at (12000, 8) with B at its floor, at (39062.5, 50) with W = 25, at (48000, 192) with tb at its floor and at (48000, 256)
with B at its ceiling and several lanes to a frame; with a slot set in mid-frame, replaced, removed and reset, a full
arena, and in a loopback from a ModBank USB station through a receiver bank's LINEAR channel.  The model runs on the
bank's own table, increment and symbol length (tests/test_psk_args.py holds them equal to the model's), so nothing in the
comparison is floating point but the quantiser's one multiply.  The traffic is what tests/test_psk_model.py shows the
model to decode."""
import functools

import numpy as np
import pytest
import torch

import psk_model as pm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import varicode
from ka9q_sdr_amd.psk import STATUS_DTYPE, STATUS_WORDS, PskBank, psk_params, status_array

pytestmark = pytest.mark.gpu

SIZES = (1, 23, 24, 25, 80, 4096, 9000)
SECONDS = 3.0
AMP = 0.1
TEXTS = ("cq cq de k1abc pse k", "the quick brown fox", "73 es gl dx test", "qrz? ur 599 in ct")


def _plan(S, bauds, per_row):
    """slot s: (row, pitch, baud, sends).  With one slot to a row every slot has a signal of its own, 0, +1 or -1 Hz off its
    pitch.  With seven to a row the slots stand 50 Hz apart and alternate between the two baud rates; an even row carries a
    signal for each of its slots of the first rate (100 Hz apart), an odd row for two of the second (200 Hz apart), and the
    other slots of a row read what those splatter."""
    out = []
    for s in range(S):
        row, j = divmod(s, per_row)
        if per_row == 1:
            out.append((row, 800.0 + 150.0 * s, bauds[s % len(bauds)], True))
        else:
            which = j % len(bauds)
            out.append((row, 700.0 + 50.0 * j + 3.0 * row, bauds[which], which == row % 2 and (which == 0 or j in (1, 5))))
    return out


@functools.lru_cache(maxsize=None)
def _rows(Fs, S, bauds, per_row):
    """the plan's rows, 3 s: every sending slot's text at amplitude 0.1 behind 16 reversals and s samples of silence; on the
    odd rows white noise at an Es/N0 of 16 dB.  ([rows][n] float32, read-only)"""
    plan = _plan(S, bauds, per_row)
    n = int(SECONDS * Fs)
    out = np.zeros((plan[-1][0] + 1, n), np.float32)
    for s, (row, pitch, baud, sends) in enumerate(plan):
        if sends:
            off = (0.0, 1.0, -1.0)[s % 3]
            x = varicode.modulate(TEXTS[s % len(TEXTS)] * 4, Fs, baud, pitch + off, AMP, lead=16)[:n - s]
            out[row, s:s + len(x)] += x
    for row in range(1, len(out), 2):
        baud = min(b for r, _, b, sends in plan if r == row and sends)
        out[row] += np.random.default_rng(300 + row).normal(0.0, pm.noise_sigma(AMP, 16.0, Fs, baud), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _models(bank, nslots, **kw):
    """a model per slot on the bank's own table, increment and symbol length"""
    table, out = bank.get_table(), []
    for s in range(nslots):
        g = bank.get_slot(s)
        out.append(pm.PskModel(bank.samprate, bank.block_len, table=table, inc=g.inc, tb=g.tb, warm=bank.warm, snr=bank.snr,
                               min_p=bank.min_p, input_scale=bank.input_scale, max_events=bank.max_events, **kw))
        assert out[-1].W == g.W
    return out


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


PARITY = [(12000.0, 24, 70, (31.25, 62.5), 7), (12000.0, 8, 3, (125.0,), 1), (39062.5, 50, 6, (31.25,), 1),
          (48000.0, 192, 3, (31.25,), 1), (48000.0, 256, 3, (10.0,), 1)]


@pytest.mark.parametrize("Fs,B,S,bauds,per_row", PARITY, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_parity_from_host_and_device_memory(gpu, Fs, B, S, bauds, per_row):
    x = _rows(Fs, S, bauds, per_row)
    n = x.shape[1]
    cuts = _chunks(n, SIZES)
    plan = _plan(S, bauds, per_row)
    want = None
    for device in (False, True):
        bank = PskBank(Fs, B, S, max(SIZES))
        for s, (row, pitch, baud, _) in enumerate(plan):
            bank.set(s, psk_params(source=row, pitch=pitch, baud=baud))
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, S), []
            for a, b in cuts:
                for m, (row, _, _, _) in zip(models, plan):
                    m.feed(x[row, a:b])
                want.append(_snap(models))
        st_t, seen = _plane(bank), [0] * S
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            st = _device_call(bank, x[:, a:b], nblocks, st_t) if device else bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, what=(device, a, b), seen=seen)
        bank.close()
    assert all(m.frames == n // B for m in models)
    assert len({m.W for m in models[:4]}) == len(bauds)      # the windows differ within a workgroup
    print("psk parity", Fs, B, S, [(m.W, m.tb, len(m.events), varicode.read_text(m.events)) for m in models[:3]])
    # the senders on the rows without noise: the text sent, as far as 3 s take it
    read = 0
    for s, (m, (row, _, baud, sends)) in enumerate(zip(models, plan)):
        if sends and row % 2 == 0:
            got, sent = varicode.read_text(m.events), TEXTS[s % len(TEXTS)] * 4
            assert len(got) >= int((SECONDS * baud - 24) / 9.0) and got == sent[:len(got)], (s, got, sent)
            read += 1
    assert read >= 2
    assert sum(len(m.events) for m in models) >= 3


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range.  Row 0 carries two
    stations, at 1000 Hz (31.25 baud) and at 2000 Hz (62.5 baud); slots 0, 1 and 3 read it at those pitches and at 5000 Hz,
    where there is only what the other two splatter; slot 2 reads row 1."""
    Fs, B = 12000.0, 12
    n = 60000
    ta, tb = "cq de k1abc", "zczc 599 001 test de w1aw"
    a = varicode.modulate(ta, Fs, 31.25, 1000.0, 0.3, lead=24)[:n]
    b = varicode.modulate(tb, Fs, 62.5, 2000.0, 0.2, lead=40)[:n]
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] += a
    x[0, :len(b)] += b
    x[1, :36000] = _rows(Fs, 2, (62.5,), 1)[1]
    x += np.random.default_rng(5).normal(0.0, 0.02, x.shape).astype(np.float32)
    loud = x * np.float32(4.0)                               # clips: (0.3 + 0.2) x 4
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = pm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    plan = [(0, 1000.0, 31.25), (0, 2000.0, 62.5), (1, 950.0, 62.5), (0, 5000.0, 31.25)]
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = PskBank(Fs, B, 4, 8192)
        for s, (r, pitch, baud) in enumerate(plan):
            bank.set(s, source=r, pitch=pitch, baud=baud)
        models = _models(bank, 4)
        assert [m.W for m in models] == [32, 16, 16, 32]
        st_t, seen = _plane(bank), [0] * 4
        for lo, hi in _chunks(n, (1000, 8192)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, (r, _, _) in zip(models, plan):
                m.feed(data[r, lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, lo, hi), seen=seen)
        bank.close()
    texts = [varicode.read_text(m.events) for m in models]   # the int16 pass: the words -32768 do no harm
    assert texts[0].startswith(ta) and texts[1].startswith(tb), texts


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves the open character alone; a removed slot stops and keeps its arena; a slot set again
    starts cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 12
    x = _rows(Fs, 2, (62.5,), 1)
    n = x.shape[1]
    first = 3 * B + 5
    bank = PskBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    rowplan = _plan(2, (62.5,), 1)
    plan = [rowplan[0], rowplan[1], rowplan[1], rowplan[0]]
    for s, r in src.items():
        bank.set(s, psk_params(r, plan[s][1], plan[s][2]))
    bank.set(2, psk_params(1, plan[2][1], plan[2][2]))       # for its increment; set again below, which is what counts
    models = _models(bank, 4)
    bank.remove(2)
    # the second call ends inside a character of slot 0, behind its fourth: found with a model of its own
    dry, cut = _models(bank, 1)[0], 0
    while not (dry.nevents >= 4 and dry.shreg):
        dry.feed(x[0, cut:cut + B])
        cut += B
    cut += 7
    assert first < cut < n - 6000
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, psk_params(1, plan[2][1], plan[2][2]))
            src[2] = 1
            models[2] = _models(bank, 4, start=first)[2]
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) >= 1
            assert int(st[0]["events"]) == 2 + int(st[0]["dropped"])
            assert int(st[0]["shreg"]) != 0, "the cut must lie inside a character for what follows to mean anything"
            bank.clear_events()
            for m in models:
                m.clear_events()
            assert not bank.counts().any()
    assert int(st[0]["dropped"]) >= 2 and int(bank.counts()[0]) == 2
    assert bank.events(0) == bank.events(3)
    assert int(st[2]["frames"]) == int(st[1]["frames"]) - 3 and int(st[2]["frames"]) == (n - 3 * B) // B
    # a removed slot stops: nothing is written for it, its arena stays; the others go on
    bank.remove(0)
    kept = bank.events(0)
    del src[0]
    st = bank.process(x[:, :cut])
    for s, r in src.items():
        models[s].feed(x[r, :cut])
    assert not st[0].tobytes().strip(b"\0") and bank.events(0) == kept and len(kept) == 2
    _check(bank, _snap(models), st, slots=list(src))
    # set again: cold, the arena empty, zeros before it on the grid that went on
    bank.set(0, psk_params(0, plan[0][1], plan[0][2]))
    assert int(bank.counts()[0]) == 0
    again = _models(bank, 1, start=n + cut)[0]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events and len(again.events) == 2
    # replaced while it runs: slot 1 takes slot 0's row and pitch and starts cold too, its arena empty; slot 0 goes on
    assert int(bank.counts()[1]) == 2
    bank.set(1, psk_params(0, plan[0][1], plan[0][2]))
    assert int(bank.counts()[1]) == 0 and bank.get_slot(1) == bank.get_slot(0)
    repl = _models(bank, 2, start=n + 2 * cut)[1]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    repl.feed(x[0, :cut])
    _check(bank, [(again.status(), again.events), (repl.status(), repl.events)], st)
    assert int(st[1]["frames"]) < int(st[0]["frames"]) and int(st[0]["dropped"]) > int(st[1]["dropped"]) >= 1
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, 4)
    src[0], src[1] = 0, 0
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, slots=list(src))
    assert bank.events(1)[0].end_sample < n
    bank.close()


# ---- loopback: a PSK31 USB station through a receiver bank's LINEAR channel, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """PSK31 audio from varicode.modulate (1500 Hz) into a USB station; a receiver bank with a LINEAR channel of 300 to
    2700 Hz at 48 kHz (an SSB passband; the bank's transform resolves 750 Hz here, so a narrower one holds no bin).  The
    decode in place on the bank's stream must read the finished plane: status and events equal what the model makes of
    the same plane pulled to the host, and the text ends with the one sent, behind a lead-in that lets the receiver's gain
    and the decoder's levels settle."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    B = 96                                                   # 16 frames in a symbol of 31.25 baud
    sent = "de K1AB 599"
    audio = varicode.modulate("cq " + sent, rate, 31.25, 1500.0, 0.5, lead=48, tail=16)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=300.0, high=2700.0, second_lo=-f))
    psk = PskBank.beside(rx, B, 1)
    assert psk.samprate == rate and psk.max_samples == per_call * La
    psk.set(0, psk_params(0, 1500.0, 31.25))
    assert psk.get_slot(0).W == 16
    model = _models(psk, 1)[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(psk.process_bank(rx))                                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = psk.events(0)
    text = varicode.read_text(got)
    print("psk loopback:", repr(text), _status(st[0]), [round(varicode.offset_hz(e, 31.25), 2) for e in got[-3:]])
    assert got == model.events
    assert text.endswith(sent), (text, got)
    for h in (mod, rx, psk):
        h.close()
