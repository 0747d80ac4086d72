"""The RTTY decoder bank (kq_rtty_*, ka9q_sdr_amd/csrc/kq_rtty.hip) on the GPU against the integer model of
tests/rtty_model.py: events (code, flags, start_sample, sig, nse), arena counts and every field of the status record -- the
counters, the framer and level state, the four window sums and the open frame's I and Q of both tones -- equal after every
call, with no tolerance anywhere.  From host and device memory, float and big-endian int16 input, padded rows, slots that
share a row at different tone pairs, calls of 1, 23, 24, 25, 80, 4096 and 9000 samples (the last is six pieces of 64
frames to a wave at B = 24), on 70 slots (18 workgroups of k_rtty, the last half empty) with two baud rates side by side, at (12000, 16) with
three (W = 17, 15 and 10 within a workgroup), at (12000, 8) with W = 30 (a history longer than an 80-sample call), at
(39062.5, 64) with a fractional bit length and at (48000, 128) with several lanes to a frame; with a slot set in
mid-frame, removed and reset, a full arena, and in a loopback from a ModBank USB station through a receiver bank's LINEAR
channel.  The model runs on the bank's own table, increments and bit length (tests/test_rtty_args.py holds them equal to
the model's), so nothing in the comparison is floating point but the quantiser's one multiply.  The traffic is what
tests/test_rtty_model.py shows the model to decode.

(12000, 24) takes 45.45 and 50 baud; 75 baud there is 6.67 frames a bit, below the floor of eight, and is refused
(tests/test_rtty_args.py), so the three rates stand side by side at (12000, 16)."""
import functools

import numpy as np
import pytest
import torch

import rtty_model as rm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import baudot
from ka9q_sdr_amd.rtty import STATUS_DTYPE, STATUS_WORDS, RttyBank, rtty_params, status_array

pytestmark = pytest.mark.gpu

SIZES = (1, 23, 24, 25, 80, 4096, 9000)
PAIRS = ((1500.0, 1670.0), (2125.0, 2295.0), (1000.0, 1450.0))       # mark, space


def _slot_plan(S, bauds):
    """slot s: (mark, space, baud, nbits)"""
    return [PAIRS[s % len(PAIRS)] + (bauds[s % len(bauds)], 5 + (s // 3) % 4 if s % 3 == 2 else 5) for s in range(S)]


@functools.lru_cache(maxsize=None)
def _rows(Fs, B, S, seconds, bauds):
    """row s: random characters back to back at slot s's tones, baud rate and character length, amplitude 0.3, behind a
    lead-in of 0.3 s of mark plus s % B samples; white noise at an Eb/N0 of 20 dB.  ([S][n] float32, read-only)"""
    n = int(seconds * Fs)
    out = np.zeros((S, n), np.float32)
    for s, (mark, space, baud, nbits) in enumerate(_slot_plan(S, bauds)):
        rng = np.random.default_rng(200 + s)
        codes = rng.integers(0, 1 << nbits, int(seconds * baud / (nbits + 2.5)) + 2).tolist()
        x = baudot.encode(codes, baud, Fs, mark, space, 0.3, nbits=nbits, lead=0.3 + (s % B) / Fs)[:n]
        out[s, :len(x)] = x
        out[s] += rng.normal(0.0, rm.noise_sigma(0.3, 20.0, Fs, baud), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _models(bank, plan, **kw):
    """a model per slot of the plan on the bank's own table, increments and bit length"""
    table, out = bank.get_table(), []
    for s, (_, _, _, nbits) in enumerate(plan):
        g = bank.get_slot(s)
        out.append(rm.RttyModel(bank.samprate, bank.block_len, nbits=nbits, table=table, incs=(g.inc_m, g.inc_s), tb=g.tb,
                                warm=bank.warm, snr=bank.snr, min_p=bank.min_p, input_scale=bank.input_scale,
                                max_events=bank.max_events, **kw))
        assert out[-1].W == g.W
    return out


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


PARITY = [(12000.0, 24, 70, 3.0, (45.45, 50.0)), (12000.0, 16, 6, 3.0, (45.45, 50.0, 75.0)), (12000.0, 8, 3, 3.0, (50.0,)),
          (39062.5, 64, 3, 2.0, (45.45,)), (48000.0, 128, 3, 2.0, (45.45,))]


@pytest.mark.parametrize("Fs,B,S,seconds,bauds", PARITY, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_parity_from_host_and_device_memory(gpu, Fs, B, S, seconds, bauds):
    x = _rows(Fs, B, S, seconds, bauds)
    n = x.shape[1]
    cuts = _chunks(n, SIZES)
    plan = _slot_plan(S, bauds)
    want = None
    for device in (False, True):
        bank = RttyBank(Fs, B, S, max(SIZES))
        for s, (mark, space, baud, nbits) in enumerate(plan):
            bank.set(s, rtty_params(source=s, mark=mark, space=space, baud=baud, nbits=nbits))
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, plan), []
            for a, b in cuts:
                for s, m in enumerate(models):
                    m.feed(x[s, a:b])
                want.append(_snap(models))
        st_t, seen = _plane(bank), [0] * S
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            st = _device_call(bank, x[:, a:b], nblocks, st_t) if device else bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, what=(device, a, b), seen=seen)
        bank.close()
    assert all(m.frames == n // B for m in models)
    assert len({m.W for m in models[:4]}) == min(len(bauds), 3 if B == 16 else 2)  # the windows differ within a workgroup
    print("rtty parity", Fs, B, S, [(m.W, m.tb, len(m.events), m.ferr) for m in models[:3]])
    # 20 dB: the characters sent, all but the one the stream ends in
    for s, m in enumerate(models):
        mark, space, baud, nbits = plan[s]
        rng = np.random.default_rng(200 + s)
        codes = rng.integers(0, 1 << nbits, int(seconds * baud / (nbits + 2.5)) + 2).tolist()
        got = [e.code for e in m.events]
        assert len(got) >= int((seconds - 0.4) * baud / (nbits + 2.5)) - 1 and got == codes[:len(got)], (s, got, codes)


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range.  Row 0 carries two
    stations, at 1000 / 1170 Hz (45.45 baud) and at 2000 / 2450 Hz (50 baud); slots 0, 1 and 3 read it at those pairs and
    at 5000 / 5170 Hz, where there is only what the other two splatter; slot 2 reads row 1."""
    Fs, B = 12000.0, 24
    n = 48000
    ta, tb = "RYRY CQ DE K1ABC", "ZCZC 599 001"
    a = baudot.encode(ta, 45.45, Fs, 1000.0, 1170.0, 0.3, lead=0.4)[:n]
    b = baudot.encode(tb, 50.0, Fs, 2000.0, 2450.0, 0.2, lead=0.45)[:n]
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] += a
    x[0, :len(b)] += b
    x[1, :36000] = _rows(Fs, B, 2, 3.0, (45.45, 50.0))[1]
    x += np.random.default_rng(5).normal(0.0, 0.02, x.shape).astype(np.float32)
    loud = x * np.float32(4.0)                               # clips: (0.3 + 0.2) x 4
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = rm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    plan = [(1000.0, 1170.0, 45.45, 5), (2000.0, 2450.0, 50.0, 5), (2125.0, 2295.0, 50.0, 5), (5000.0, 5170.0, 45.45, 5)]
    src = (0, 0, 1, 0)
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = RttyBank(Fs, B, 4, 8192)
        for s, ((mark, space, baud, nbits), r) in enumerate(zip(plan, src)):
            bank.set(s, source=r, mark=mark, space=space, baud=baud, nbits=nbits)
        models = _models(bank, plan)
        st_t, seen = _plane(bank), [0] * 4
        for lo, hi in _chunks(n, (1000, 8192)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, r in zip(models, src):
                m.feed(data[r, lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, lo, hi), seen=seen)
        bank.close()
    texts = [baudot.read_text(m.events) for m in models]     # the int16 pass: the words -32768 do no harm
    assert texts[0].startswith(ta) and texts[1].startswith(tb), texts


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves the open character alone; a removed slot stops and keeps its arena; a slot set again
    starts cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 24
    bauds = (45.45, 50.0)
    x = _rows(Fs, B, 2, 3.0, bauds)
    n = x.shape[1]
    first = 3 * B + 17
    bank = RttyBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    rowplan = _slot_plan(2, bauds)
    plan = [rowplan[0], rowplan[1], rowplan[1], rowplan[0]]
    for s, r in src.items():
        bank.set(s, rtty_params(r, *plan[s]))
    bank.set(2, rtty_params(1, *plan[2]))                    # for its increments; set again below, which is what counts
    models = _models(bank, plan)
    bank.remove(2)
    cut = 18000 + 7
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, rtty_params(1, *plan[2]))
            src[2] = 1
            models[2] = _models(bank, plan, start=first)[2]
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) >= 1
            assert int(st[0]["events"]) == 2 + int(st[0]["dropped"])
            assert int(st[0]["state"]) == rm.CHAR, "the cut must lie inside a character for what follows to mean anything"
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
    bank.set(0, rtty_params(0, *plan[0]))
    assert int(bank.counts()[0]) == 0
    again = _models(bank, plan, start=n + cut)[0]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events and len(again.events) == 2
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, plan)
    src[0] = 0
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, slots=list(src))
    assert bank.events(1)[0].start_sample < n
    bank.close()


# ---- loopback: an FSK-keyed USB station through a receiver bank's LINEAR channel, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """Teleprinter audio from baudot.encode (45.45 baud, 1500 / 1670 Hz) into a USB station; a receiver bank with a LINEAR
    channel of 1300 to 1870 Hz at 48 kHz.  The decode in place on the bank's stream must read the finished plane: status and
    events equal what the model makes of the same plane pulled to the host, and the text ends with the one sent, behind an
    RYRY that lets the receiver's gain and the decoder's levels settle."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    B = 96                                                   # 11 frames in a bit of 45.45 baud
    sent = "K1AB 59"
    audio = baudot.encode("RYRY " + sent, 45.45, rate, 1500.0, 1670.0, 0.5, lead=0.5, tail=0.2)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=1300.0, high=1870.0, second_lo=-f))
    tty = RttyBank.beside(rx, B, 1)
    assert tty.samprate == rate and tty.max_samples == per_call * La
    plan = [(1500.0, 1670.0, 45.45, 5)]
    tty.set(0, rtty_params(0, *plan[0]))
    assert tty.get_slot(0).W == 11
    model = _models(tty, plan)[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(tty.process_bank(rx))                                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = tty.events(0)
    text = baudot.read_text(got)
    print("rtty loopback:", repr(text), _status(st[0]))
    assert got == model.events
    assert text.endswith(sent), (text, got)
    for h in (mod, rx, tty):
        h.close()
