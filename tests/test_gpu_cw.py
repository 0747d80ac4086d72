"""The CW decoder bank (kq_cw_*, ka9q_sdr_amd/csrc/kq_cw.hip) on the GPU against the integer model of tests/cw_model.py:
events (code, nelem, unit, start_sample, end_sample, peak), arena counts and every field of the status record -- the
counters, the whole tracker state and the open frame's I and Q, which is all that is carried from call to call -- equal
after every call, with no tolerance anywhere.  From host and device memory, float and big-endian int16 input, padded rows,
slots that share a row at different pitches, calls of 1, 47, 48, 49, 80, 4096 and 9000 samples (the last longer than a
staging piece), on 70 slots (18 workgroups of k_cw, the last half empty), at (39062.5, 128) and with B = 1024 (16
lanes to a frame at the least, frames that span many calls), with a slot set in mid-frame, removed and reset, a full
arena, and in a loopback from a ModBank USB station through a receiver bank's CW channel.  The model runs on the bank's
own table and increments (tests/test_cw_args.py holds them equal to the model's), so nothing in the comparison is floating
point but the quantiser's one multiply.  The traffic is what tests/test_cw_model.py shows the model to decode."""
import functools

import numpy as np
import pytest
import torch

import cw_model as cm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import morse
from ka9q_sdr_amd.cw import STATUS_DTYPE, STATUS_WORDS, CwBank, cw_params, status_array

pytestmark = pytest.mark.gpu

WORDS = ("CQ K1ABC", "DE W9XYZ", "5NN TU", "73 SK", "QRZ?", "PSE K", "TEST N0AX")
SPEEDS = (20.0, 25.0, 32.0)
SIZES = (1, 47, 48, 49, 80, 4096, 9000)


@functools.lru_cache(maxsize=None)
def _rows(Fs, B, S, seconds, wpms=SPEEDS):
    """row s: WORDS[s % 7] over and over at wpms[s % 3], 700 Hz, amplitude 0.3, from a lead-in of 0.3 s plus s % B samples;
    white noise 20 dB down in Fs / B.  ([S][n] float32, read-only)"""
    n = int(seconds * Fs)
    out = np.zeros((S, n), np.float32)
    for s in range(S):
        x = morse.encode(" ".join([WORDS[s % len(WORDS)]] * 8), wpms[s % len(wpms)], Fs, 700.0, 0.3, lead=0.3 + (s % B) / Fs)
        x = x[:n]
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(100 + s).normal(0.0, cm.noise_sigma(0.3, 20.0, B), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _models(bank, slots, cfg, **kw):
    """a model per (slot, pitch, wpm) on the bank's own table and increment"""
    table = bank.get_table()
    return [cm.CwModel(bank.samprate, bank.block_len, wpm=w, table=table, inc=bank.get_inc(s), input_scale=bank.input_scale,
                       max_events=bank.max_events, **cfg, **kw) for s, _, w in slots]


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


SLOW = dict(min_wpm=2.0, max_wpm=15.0, warm=16)             # frames of 21 ms: 64 of them would train the floor on the traffic
PARITY = [(12000.0, 48, 70, 3.0, {}, SPEEDS), (12000.0, 48, 3, 3.0, {}, SPEEDS), (39062.5, 128, 3, 3.0, {}, SPEEDS),
          (48000.0, 1024, 3, 6.0, SLOW, (8.0, 10.0, 13.0))]


@pytest.mark.parametrize("Fs,B,S,seconds,cfg,wpms", PARITY, ids=lambda v: str(v) if not isinstance(v, (dict, tuple)) else "")
def test_parity_from_host_and_device_memory(gpu, Fs, B, S, seconds, cfg, wpms):
    x = _rows(Fs, B, S, seconds, wpms)
    n = x.shape[1]
    cuts = _chunks(n, SIZES)
    slots = [(s, 700.0, wpms[(s + 1) % 3]) for s in range(S)]                 # start speeds one step off the sender's
    want = None
    for device in (False, True):
        bank = CwBank(Fs, B, S, max(SIZES), **cfg)
        for s, pitch, wpm in slots:
            bank.set(s, cw_params(source=s, pitch=pitch, wpm=wpm))
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, slots, cfg), []
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
    texts = [morse.read_text(m.events) for m in models]
    print("cw parity", Fs, B, S, texts[:3])
    assert sum(len([e for e in m.events if e.code > 1]) for m in models) >= (3 * S if B < 1024 else S)
    if B == 48:       # 3 s hold four or five characters: those sent, where the start speed is within 1.4 of the sender's
        for s, t in enumerate(texts):
            assert s % 3 == 2 or (len(t) >= 2 and " ".join([WORDS[s % len(WORDS)]] * 8).startswith(t)), (s, t)


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range.  Row 0 carries two
    stations, at 400 and 900 Hz (two frame bandwidths of 250 Hz apart); slots 0, 1 and 3 read it at 400, 900 and 650 Hz,
    slot 2 reads row 1 at 700 Hz."""
    Fs, B = 12000.0, 48
    n = 60000
    a = morse.encode("CQ K1ABC", 30.0, Fs, 400.0, 0.3, lead=0.3)[:n]
    b = morse.encode("TEST W9", 22.0, Fs, 900.0, 0.2, lead=0.35)[:n]
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] += a
    x[0, :len(b)] += b
    x[1] = _rows(Fs, B, 2, 5.0)[1]
    x += np.random.default_rng(5).normal(0.0, 0.003, x.shape).astype(np.float32)
    loud = x * np.float32(4.0)                               # clips where both stations are keyed: (0.3 + 0.2) x 4
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = cm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    slots = [(0, 400.0, 25.0), (1, 900.0, 25.0), (2, 700.0, 25.0), (3, 650.0, 25.0)]
    src = (0, 0, 1, 0)
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = CwBank(Fs, B, 4, 8192)
        for (s, pitch, wpm), r in zip(slots, src):
            bank.set(s, source=r, pitch=pitch, wpm=wpm)
        models = _models(bank, slots, {})
        st_t, seen = _plane(bank), [0] * 4
        for lo, hi in _chunks(n, (1000, 8192)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, r in zip(models, src):
                m.feed(data[r, lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, lo, hi), seen=seen)
        bank.close()
    texts = [morse.read_text(m.events) for m in models]      # the int16 pass: the words -32768 do no harm
    assert "CQ K1ABC" in texts[0] and "TEST W9" in texts[1], texts
    # 250 Hz off both stations, in the nulls of a frame's response (between the frames that hold the words -32768)
    assert max(models[3].P[3:-1]) < max(models[0].P[3:-1]) // 16


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves the open character alone; a removed slot stops and keeps its arena; a slot set again
    starts cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 48
    x = _rows(Fs, B, 2, 5.0)
    n = x.shape[1]
    first = 3 * B + 17
    bank = CwBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    slots = [(s, 700.0, 25.0) for s in range(4)]
    for s, r in src.items():
        bank.set(s, cw_params(source=r, pitch=700.0, wpm=25.0))
    bank.set(2, source=1, pitch=650.0, wpm=25.0)             # for its increment; set again below, which is what counts
    models = _models(bank, slots, {})
    bank.remove(2)
    cut = 30000
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, source=1, pitch=700.0, wpm=25.0)
            src[2] = 1
            models[2] = _models(bank, slots, {}, start=first)[2]
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) >= 1
            assert int(st[0]["events"]) == 2 + int(st[0]["dropped"])
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
    bank.set(0, source=0, pitch=700.0, wpm=25.0)
    assert int(bank.counts()[0]) == 0
    again = _models(bank, slots, {}, start=n + cut)[0]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, slots, {})
    src[0] = 0
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, slots=list(src))
    assert bank.events(1)[0].start_sample < n
    bank.close()


def test_cold_start_of_slots_set_before_the_first_call(gpu):
    """Slots set before the first call reach the device in runs (0 to 2 together, 4 alone; 3 was set and removed again):
    each starts from its own dot length u0, an empty character with both gaps reported, and an empty arena, and the slots
    never set stay all zero.  After reset() the same holds for a slot set anew at another speed."""
    Fs, B, S = 12000.0, 48, 8
    u_min, u_max = cm.unit_limits(Fs, B, 5.0, 60.0)
    u0 = lambda wpm: min(max(cm.unit_start(Fs, B, wpm), u_min), u_max)
    wpm = {0: 12.0, 1: 20.0, 2: 25.0, 4: 32.0}
    bank = CwBank(Fs, B, S, 2 * B)
    for s, w in wpm.items():
        bank.set(s, source=0, pitch=700.0, wpm=w)
    bank.set(3, source=0, pitch=700.0, wpm=40.0)
    bank.remove(3)
    assert len({u0(w) for w in wpm.values()}) == 4
    zeros = np.zeros((1, 2 * B), np.float32)

    def check(st):
        for s in range(S):
            if s in wpm:
                assert (int(st[s]["unit"]), int(st[s]["code"]), int(st[s]["flags"]), int(st[s]["frames"])) == (u0(wpm[s]), 1, 3, 2), s
            else:
                assert not st[s].tobytes().strip(b"\0"), s
        assert not bank.counts().any()

    check(bank.process(zeros))
    bank.reset()
    wpm[2] = 16.0
    bank.set(2, source=0, pitch=700.0, wpm=wpm[2])
    check(bank.process(zeros))
    bank.close()


# ---- loopback: a keyed USB station through a receiver bank's CW channel, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """Morse from morse.encode as a 700 Hz tone into a USB station; a receiver bank with a LINEAR channel of 500 to 900 Hz
    (CWU: +-200 Hz about the 700 Hz pitch) at 48 kHz.  The decode in place on the bank's stream must read the finished
    plane: status and events equal what the model makes of the same plane pulled to the host, and the text is the one
    sent, behind a VVV that lets the receiver's gain and the decoder's floor settle."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    B = 192
    sent = "K1AB"
    audio = morse.encode("VVV " + sent, 35.0, rate, 700.0, 0.5, lead=0.3)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=500.0, high=900.0, second_lo=-f))
    cw = CwBank.beside(rx, B, 1)
    assert cw.samprate == rate and cw.max_samples == per_call * La
    cw.set(0, source=0, pitch=700.0, wpm=25.0)
    model = _models(cw, [(0, 700.0, 25.0)], {})[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(cw.process_bank(rx))                                    # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = cw.events(0)
    text = morse.read_text(got)
    print("cw loopback:", repr(text), _status(st[0]))
    assert got == model.events
    assert text.endswith(sent), (text, got)
    for h in (mod, rx, cw):
        h.close()
