"""The tone signalling decoder bank (kq_tone_*, ka9q_sdr_amd/csrc/kq_tone.hip) on the GPU against the integer model of
tests/tone_model.py: events (symbol, blocks, start_sample, peak), arena counts, every status field and the powers plane
(the P_t and E of the last completed block, which pins the correlators themselves) equal after every call, with no
tolerance anywhere -- from host and device memory, float and big-endian int16 input, padded rows, two slots on one row,
under other call splits, on 70 slots (70 workgroups of k_tone), at the largest sums the limits allow (B = 8 with 32 tones,
B = 4096 with one tone on full-scale input), with a slot set in mid-block, removed and reset, a full arena, a run open
across calls, and in a loopback from a ModBank FM station through a receiver bank's channel.  The model runs on the bank's
own table and increments (tests/test_tone_args.py holds them equal to the model's), so nothing in the comparison is
floating point but the quantiser's one multiply.  The DTMF and ZVEI1 trains are those tests/test_tone_model.py shows the
model to decode completely, so the events must also be the keys sent."""
import functools

import numpy as np
import pytest
import torch

import bank_gpu
import ka9q_sdr_amd as kq
import tone_model as tm
from ka9q_sdr_amd import selcall as sc
from ka9q_sdr_amd.tone import STATUS_DTYPE, STATUS_WORDS, ToneBank, status_array, tone_params

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rows(Fs, B, plan, S):
    """slot s's train (seed s % 20, as the CPU test's; twist -4, 0, +4 dB in turn), zeros behind the shorter ones"""
    if plan is sc.DTMF:
        trains = [tm.dtmf_train(Fs, B, 1000 + s % 20, (-4.0, 0.0, 4.0)[s % 3]) for s in range(S)]
    else:
        trains = [tm.zvei_train(Fs, B, s % 20, plan) for s in range(S)]
    n = max(len(x) for _, _, x in trains)
    x = np.array([np.concatenate([x, np.zeros(n - len(x), np.float32)]) for _, _, x in trains])
    x.setflags(write=False)
    return [k for k, _, _ in trains], x


def _bank(Fs, cfg, S, max_samples, **kw):
    return ToneBank(Fs, max_slots=S, max_samples=max_samples, **cfg, **kw)


def _models(bank, n, cfg, **kw):
    table, incs = bank.get_table(), bank.get_incs()
    return [tm.ToneModel(bank.samprate, table=table, incs=incs, input_scale=bank.input_scale, max_events=bank.max_events,
                         **cfg, **kw) for _ in range(n)]


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events", planes=("powers",)), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


def _planes(bank):
    """status and powers planes on the device, the powers' rows one value longer than they need be"""
    return _plane(bank), torch.zeros((bank.max_slots, bank.ntones + 2), dtype=torch.int64, device="cuda")


def _powers(bank, pw):
    return pw.cpu().numpy().view(np.uint64)[:, :bank.ntones + 1]


def _sent(plan, events, B):
    if plan is sc.DTMF:
        return "".join(k.key for k in sc.read_dtmf(events, B))
    calls = sc.read_sequence(events, B, plan)
    return calls[0].digits if len(calls) == 1 else calls


PARITY = [(8000.0, 102, sc.DTMF, 70), (48000.0, 612, sc.DTMF, 3), (39062.5, 500, sc.ZVEI1, 3)]


@pytest.mark.parametrize("Fs,B,plan,S", PARITY, ids=lambda v: getattr(v, "name", str(v)))
def test_parity_from_host_and_device_memory(gpu, Fs, B, plan, S):
    sent, x = _rows(Fs, B, plan, S)
    cfg = sc.plan_config(plan, Fs, block_len=B)
    n = x.shape[1]
    cap = n // 3 + 64
    cuts = _chunks(n, (cap, 257, n // 4))                    # several calls, ending inside blocks
    want = None
    for device in (False, True):
        bank = _bank(Fs, cfg, S, cap)
        for s in range(S):
            bank.set(s, tone_params(source=s))
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, S, cfg), []
            for a, b in cuts:
                for s, m in enumerate(models):
                    m.feed(x[s, a:b])
                want.append(_snap(models))
        st_t, pw_t = _planes(bank)
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            if device:
                st = _device_call(bank, x[:, a:b], nblocks, st_t, extra=(pw_t.data_ptr(), pw_t.shape[1]))
                pw = _powers(bank, pw_t)
            else:
                st, pw = bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, pw, what=(device, a, b))
        bank.close()
    assert [_sent(plan, m.events, B) for m in models] == sent
    assert all(m.blocks == n // B and m.valid >= 10 for m in models)


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range; slots 0 and 2 read
    row 0"""
    Fs, B = 8000.0, 102
    cfg = sc.plan_config(sc.DTMF, Fs)
    sent, x = _rows(Fs, B, sc.DTMF, 2)
    loud = x * np.float32(6.0)                               # clips: low + high tone reach 0.65 x 6
    assert (np.abs(loud) * 32767 > 32767).mean() > 0.2
    words = tm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768                               # in the silence ahead of the first key
    words[0, -3:] = -32768
    src = (0, 1, 0)
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = _bank(Fs, cfg, 3, 8192)
        for s, r in enumerate(src):
            bank.set(s, source=r)
        models = _models(bank, 3, cfg)
        st_t, pw_t = _planes(bank)
        for a, b in _chunks(x.shape[1], (1000, 8192)):
            if device:
                st = _device_call(bank, data[:, a:b], 1, st_t, fmt, extra=(pw_t.data_ptr(), pw_t.shape[1]))
                pw = _powers(bank, pw_t)
            else:
                st, pw = bank.process(data[:, a:b], 1, fmt)
            for m, r in zip(models, src):
                m.feed(data[r, a:b], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, pw, what=(fmt, a, b))
        assert bank.events(0) == bank.events(2) and len(bank.events(0)) > 0
        bank.close()
    assert [_sent(sc.DTMF, m.events, B) for m in models[:2]] == sent       # the int16 pass: the words -32768 do no harm


def test_call_splits_change_nothing(gpu):
    """the stream cut in turn into calls of 1, 63, 64, 65, B - 1, B, B + 1, 1000 and 7777 samples, in one block or many:
    the model's records after every call, and at the end those of the model fed in one piece"""
    Fs, B, S = 8000.0, 102, 3
    cfg = sc.plan_config(sc.DTMF, Fs)
    sent, x = _rows(Fs, B, sc.DTMF, S)
    n = x.shape[1]
    whole = _snap([tm.ToneModel(Fs, **cfg).feed(x[s]) for s in range(S)])
    for sizes in ((1, 63, 64, 65, B - 1, B, B + 1, 1000, 7777), (n,), (2 * B, 2049, 7, 4 * B + 1)):
        bank = _bank(Fs, cfg, S, n)
        for s in range(S):
            bank.set(s, source=s)
        models = _models(bank, S, cfg)
        for a, b in _chunks(n, sizes):
            m = b - a
            st, pw = bank.process(x[:, a:b], next(k for k in (8, 3, 2, 1) if m % k == 0))
            for s in range(S):
                models[s].feed(x[s, a:b])
            _check(bank, _snap(models), st, pw, what=(sizes, a, b))
        _check(bank, whole, st, pw, what=sizes)
        bank.close()
    assert [_sent(sc.DTMF, w[2], B) for w in whole] == sent


def test_largest_sums(gpu):
    """B = 4096, one tone, q = +-32767 in phase with it (|I| just below 2^42, P near 2^53, E B near 2^54); and B = 8 with
    32 tones in two groups on noise and a tone.  Calls that end inside blocks and span several."""
    Fs, B = 48000.0, 4096
    cfg = dict(block_len=B, freqs=(1000.0,), groups=(1,), frac=100, ratio=4095, twist=4095, min_blocks=1, min_ms=32767 ** 2)
    bank = _bank(Fs, cfg, 2, 3 * B, max_events=4)
    bank.set(0, source=0)
    bank.set(1, source=0)
    models = _models(bank, 2, cfg)
    j = ((np.arange(5 * B, dtype=np.uint64) * np.uint64(bank.get_incs()[0])) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)
    q = np.where(bank.get_table()[j.astype(np.int64)] >= 0, 32767, -32768).astype(np.int16)[None, :]
    q[0, 4 * B + 100:] = 0                                   # the run of symbol 0 ends in block 4
    for a, b in _chunks(5 * B, (B + 1000, 3 * B, 77)):
        st, pw = bank.process(q[:, a:b], 1, kq.KQ_PCM_S16BE)
        for m in models:
            m.feed(q[0, a:b], s16=True)
        _check(bank, _snap(models), st, pw, what=(a, b))
    assert int(pw[0, 1]) < B * 32767 ** 2 and models[0].events == [tm.Event(0, 4, 0, B * 32767 ** 2)]
    assert max(models[0].widest) > 2 ** 53 and int(st[0]["valid_blocks"]) == 4
    bank.close()
    Fs, B = 8000.0, 8
    freqs = tuple(np.linspace(300.0, 3400.0, 32))
    cfg = dict(block_len=B, freqs=freqs, groups=(13, 19), frac=1, ratio=16, twist=4095, min_blocks=1, min_ms=0)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.2, 1.2, (2, 1000)).astype(np.float32)
    x[1] = 0.9 * np.sin(2 * np.pi * freqs[20] / Fs * np.arange(1000))
    bank = _bank(Fs, cfg, 2, 1000, max_events=64)
    for s in range(2):
        bank.set(s, source=s)
    models = _models(bank, 2, cfg)
    for a, b in _chunks(1000, (3, B, 321, 63)):
        st, pw = bank.process(x[:, a:b])
        for s in range(2):
            models[s].feed(x[s, a:b])
        _check(bank, _snap(models), st, pw, what=(a, b))
    assert int(st[0]["blocks"]) == 125 and int(st[0]["dropped"]) > 0 and int(st[0]["valid_blocks"]) > 60
    bank.close()


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside block 1 and sees zeros before it; an arena of three events fills and counts what it drops;
    clear_events empties it and leaves the open run alone; a key lies across a call boundary: open in the status, no event
    yet; a removed slot stops and keeps its arena; reset starts the grid over"""
    Fs, B = 8000.0, 102
    cfg = sc.plan_config(sc.DTMF, Fs)
    sent, x = _rows(Fs, B, sc.DTMF, 2)
    n = x.shape[1]
    first = 150
    bank = _bank(Fs, cfg, 4, n, max_events=3)
    src = {0: 0, 1: 1, 3: 0}
    for s, r in src.items():
        bank.set(s, tone_params(source=r))
    models = _models(bank, 4, cfg)
    late = _models(bank, 1, cfg, start=first)[0]
    key3 = int((float(tm.dtmf_train(Fs, B, 1000, -4.0)[1]) + 0.3) * Fs) + 200     # half way through row 0's fourth key
    for a, b in ((0, first), (first, key3), (key3, n)):
        st, pw = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, pw, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0") and not pw[2].any()
            bank.set(2, source=1)
            src[2] = 1
            models[2] = late
        if b == key3:                                        # three keys closed; the fourth is open, and no event yet
            assert int(bank.counts()[0]) == 3 and int(st[0]["cur"]) >= 0 and int(st[0]["run"]) >= 1
            assert sc.symbol_key(sc.DTMF, int(st[0]["cur"])) == sent[0][3]
            bank.clear_events()
            for m in models:
                m.clear_events()
            assert not bank.counts().any()
    assert (int(st[0]["events"]), int(st[0]["dropped"]), int(bank.counts()[0])) == (16, 10, 3)
    assert "".join(k.key for k in sc.read_dtmf(bank.events(0), B)) == sent[0][3:6]          # the open run went on
    assert bank.events(0) == bank.events(3) and bank.events(2) == bank.events(1)            # nothing before sample 150
    assert int(st[2]["blocks"]) == int(st[1]["blocks"]) - 1
    # a removed slot stops: nothing is written for it, its arena stays; the others go on
    bank.remove(0)
    kept = bank.events(0)
    del src[0]
    st, pw = bank.process(x)
    for s, r in src.items():
        models[s].feed(x[r])
    assert not st[0].tobytes().strip(b"\0") and not pw[0].any() and bank.events(0) == kept
    _check(bank, _snap(models), st, pw, slots=list(src))
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, 4, cfg)
    st, pw = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, pw, slots=list(src))
    assert bank.events(1)[0].start_sample < n and bank.events(0) == kept
    bank.close()


# ---- loopback: an FM station through a receiver bank, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """DTMF keys from dtmf_encode on an FM station of 3 kHz deviation; a receiver bank with a flat FM channel at 48 kHz
    (its output is rad/sample: 2 pi 3000 / 48000 = 0.39 at full deviation, so input_scale 65534 brings the 0.25 + 0.25
    of the two tones to +-6400).  The decode in place on the bank's stream must read the finished plane: status, powers
    and events equal what the model makes of the same plane pulled to the host, and the keys are those sent."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    keys = "147#0D"
    audio = sc.dtmf_encode(keys, rate, lead=0.03, tail=0.08)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("fm", frequency=f, amplitude_dbfs=-20.0, deviation=3000.0, low=-7000.0, high=7000.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-10000.0, high=10000.0, second_lo=-f, flat=1))
    cfg = sc.plan_config(sc.DTMF, rate)
    tone = ToneBank.beside(rx, max_slots=1, input_scale=65534.0, **cfg)
    assert tone.samprate == rate and tone.max_samples == per_call * La and tone.block_len == 612
    tone.set(0, source=0)
    model = _models(tone, 1, cfg)[0]
    pw_t = torch.zeros((1, tone.ntones + 1), dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        # receiver noise as in test_gpu_pag's loopback: it keeps the squelch's amplitude variance above zero
        noisy = s16.astype(np.float64) + rng.normal(0.0, 200.0, s16.shape)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(tone.process_bank(rx, powers=pw_t))                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
        assert [int(v) for v in pw_t.cpu().numpy()[0]] == model.powers(), c
    print("tone loopback:", _status(st[0]))
    got = tone.events(0)
    assert got == model.events
    assert "".join(k.key for k in sc.read_dtmf(got, 612)) == keys, (got, _status(st[0]))
    for h in (mod, rx, tone):
        h.close()
