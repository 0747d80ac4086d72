"""The ALE decoder bank (kq_ale_*, ka9q_sdr_amd/csrc/kq_ale.hip) on the GPU against the integer model of tests/ale_model.py:
events (word, flags, err_a, err_b, split, end_sample, sig, nse), arena counts and every field of the status record -- the
counters, the clock, the early, centre and late powers, the levels, the tone, the 147-bit register, word sync, the sixteen
window sums and the open frame's I and Q per tone -- equal after every call, with no tolerance anywhere.  From host and
device memory, float and big-endian int16 input, padded rows, calls of 1, 23, 24, 25, 80, 4096 and 9000 samples, on 70 slots
(18 workgroups of k_ale, the last half empty) that share rows with f0 40 Hz off either way, half a tone and a tone off and
with a negative df (READS says which of them read the words, and why); at (8000, 8) with W = 8, at (12000, 8) with W = 12 and a call of 80 samples shorter than the
window of 96, at (39062.5, 32) with a fractional symbol and at (96000, 96) with two lanes to a frame; with a slot set in
mid-frame, removed and reset, a full arena, word sync lost and regained, and in a loopback from a ModBank USB station
through a receiver bank's LINEAR channel.  The model runs on the bank's own table, increments and symbol length
(tests/test_ale_args.py holds them equal to the model's), so nothing in the comparison is floating point but the
quantiser's one multiply.  The traffic is what tests/test_ale_model.py shows the model to decode."""
import functools

import numpy as np
import pytest
import torch

import ale_model as am
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import ale2g
from ka9q_sdr_amd.ale import STATUS_DTYPE, STATUS_WORDS, AleBank, ale_params, status_array

pytestmark = pytest.mark.gpu

SIZES = (1, 23, 24, 25, 80, 4096, 9000)
AMP = 0.1
LEAD = [ale2g.word("TO", "ABC")] * 4
PAYLOAD = ([ale2g.word("TO", "ABC"), ale2g.word("TIS", "XY1"), ale2g.word("CMD", "a~\x05"), ale2g.word("DATA", "2@@"),
            ale2g.word("TWAS", "K1A"), ale2g.word("REP", "BC?")],
           [ale2g.word("FROM", "N0C"), ale2g.word("THRU", "ALL"), ale2g.word("TO", "W1A"), ale2g.word("DATA", "W@@"),
            ale2g.word("CMD", "\x7f\x00z"), ale2g.word("TIS", "909")])
BURST_WORD = 8                                              # the word of a row whose copies are hit: the fifth of the payload
# (f0, df): the signal's own tone plan; 40 Hz above and below it; the plan upside down (tone t where 7 - t is sent); the
# signal's own again; half a tone and a whole tone above it.  What each must read is worked out at RIGHT below.
VARIANTS = ((750.0, 250.0), (790.0, 250.0), (710.0, 250.0), (2500.0, -250.0), (750.0, 250.0), (875.0, 250.0), (1000.0, 250.0))
# Which plans read the words.  40 Hz off, the tone sent still lies in the main lobe of its own correlator (a symbol of 8 ms
# has its first null 125 Hz away) at sinc^2(0.32) = 0.72 of its power, with 0.03 at most in any other: the decision does
# not change, so these slots read what the right one reads -- 8-FSK at 250 Hz spacing cannot tell 40 Hz of mistuning, and
# a decoder that could would not copy a station that far off.  Upside down, tone 7 - t carries t's three bits with the
# highest inverted (the Gray map is reflected); 49 is 1 mod 3, so the inverted place moves by one from copy to copy, every
# place of the 49 is wrong in exactly one copy, and the vote mends all of it: the words are read, with split = 49.  Half a
# tone off the two neighbours tie, and a whole tone off every tone is read as its neighbour: neither files a word of the
# payload.
READS = (True, True, True, True, True, False, False)


@functools.lru_cache(maxsize=None)
def _rows(Fs):
    """two rows of about 4 s: four lead-in words and six payload words at amplitude 0.1 behind 30 symbols of silence; in
    word 8 each of the three copies is hit by a burst of three wrong tones of its own, at another place of the copy; row 1
    carries white noise at an Es/N0 of 14 dB.  ([2][n] float32, read-only)"""
    out = []
    for r in range(2):
        sym = ale2g.word_symbols(LEAD + list(PAYLOAD[r]))
        for at in (1, 23, 44):                               # bits 3.., 49 + 20.., 98 + 34..: other bits of every copy
            sym[49 * BURST_WORD + at:49 * BURST_WORD + at + 3] = (sym[49 * BURST_WORD + at:49 * BURST_WORD + at + 3] + 3) % 8
        out.append(ale2g.modulate_symbols(sym, Fs, amp=AMP, lead=30 + 0.3 * r, tail=10))
    n = max(len(x) for x in out)
    x = np.zeros((2, n), np.float32)
    for r in range(2):
        x[r, :len(out[r])] = out[r]
    x[1] += np.random.default_rng(400).normal(0.0, am.noise_sigma(AMP, 14.0, Fs), n).astype(np.float32)
    x.setflags(write=False)
    return x


def _plan(S):
    """slot s: (row, kind, f0, df).  Seven slots to a row, one of each variant; the rows 0, 2, .. carry the first signal, the
    rows 1, 3, .. the second, so slots a multiple of 14 apart read the same samples with the same plan"""
    return [(s // 7, (s // 7 % 2, s % 7)) + VARIANTS[s % 7] for s in range(S)]


def _model(bank, slot, **kw):
    """a model on the bank's own table, increments and symbol length"""
    g = bank.get_slot(slot)
    m = am.AleModel(bank.samprate, bank.block_len, table=bank.get_table(), inc=g.inc, tb=g.tb, warm=bank.warm, snr=bank.snr,
                    min_p=bank.min_p, acq_err=bank.acq_err, lose=bank.lose, input_scale=bank.input_scale,
                    max_events=bank.max_events, **kw)
    assert m.W == g.W
    return m


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap_one, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


PARITY = [(8000.0, 8, 70), (12000.0, 8, 3), (39062.5, 32, 3), (96000.0, 96, 4)]


@pytest.mark.parametrize("Fs,B,S", PARITY)
def test_parity_from_host_and_device_memory(gpu, Fs, B, S):
    base = _rows(Fs)
    plan = _plan(S)
    x = base[[r % 2 for r in range(plan[-1][0] + 1)]]
    n = x.shape[1]
    cuts = _chunks(n, SIZES)
    want = None
    for device in (False, True):
        bank = AleBank(Fs, B, S, max(SIZES))
        for s, (row, _, f0, df) in enumerate(plan):
            bank.set(s, ale_params(source=row, f0=f0, df=df))
        if want is None:                                     # the models' records after every call, made once per kind
            kinds = {kind: s for s, (_, kind, _, _) in reversed(list(enumerate(plan)))}
            models = {kind: _model(bank, s) for kind, s in kinds.items()}
            assert all(bank.get_slot(s) == bank.get_slot(kinds[kind]) for s, (_, kind, _, _) in enumerate(plan))
            want = []
            for a, b in cuts:
                for (r, _), m in models.items():
                    m.feed(base[r, a:b])
                snap = {kind: _snap(m) for kind, m in models.items()}
                want.append([snap[kind] for _, kind, _, _ in plan])
        st_t, seen = _plane(bank), [0] * S
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            st = _device_call(bank, x[:, a:b], nblocks, st_t) if device else bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, what=(device, a, b), seen=seen)
        bank.close()
    assert all(m.frames == n // B for m in models.values())
    print("ale parity", Fs, B, S, models[(0, 0)].W, models[(0, 0)].tb, [(k, len(m.events)) for k, m in sorted(models.items())])
    for r in sorted({r for r, _ in models}):                  # the right slot reads its row's payload whole, the burst word too
        m = models[(r, 0)]
        got = [e.word for e in m.events if not e.flags]
        assert got[-6:] == list(PAYLOAD[r]), (r, ale2g.read(m.events))
        hit = [e for e in m.events if e.word == PAYLOAD[r][BURST_WORD - 4]][-1]
        assert hit.split >= 9 and hit.err_a + hit.err_b <= 2, hit
    for (r, v), m in models.items():                          # and the other plans: READS
        got = [e.word for e in m.events if not e.flags]
        if READS[v] and VARIANTS[v][1] > 0:
            assert got[-6:] == list(PAYLOAD[r]), ((r, v), ale2g.read(m.events))
        elif READS[v]:                                       # upside down the vote has nothing left for the burst word
            assert set(PAYLOAD[r]) - {PAYLOAD[r][BURST_WORD - 4]} <= set(got), ((r, v), ale2g.read(m.events))
            clean = set(LEAD + list(PAYLOAD[r])) - {PAYLOAD[r][BURST_WORD - 4]}
            assert all(e.split >= 45 for e in m.events if e.word in clean)   # 49, less what noise turns back
        else:
            assert not set(got) & set(PAYLOAD[r]), ((r, v), ale2g.read(m.events))


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range; slots 0 and 1 read
    the two rows, slot 2 row 0 and slot 3 row 1 a tone off"""
    Fs, B = 12000.0, 12
    base = _rows(Fs)
    n = 30000
    x = base[:, :n] * np.float32(4.0) + np.random.default_rng(5).normal(0.0, 0.02, (2, n)).astype(np.float32)
    loud = x * np.float32(3.0)                               # clips: 0.1 x 12
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = am.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    plan = [(0, 750.0, 250.0), (1, 750.0, 250.0), (0, 1000.0, 250.0), (1, 500.0, 250.0)]
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = AleBank(Fs, B, 4, 8192)
        for s, (r, f0, df) in enumerate(plan):
            bank.set(s, source=r, f0=f0, df=df)
        models = [_model(bank, s) for s in range(4)]
        st_t, seen = _plane(bank), [0] * 4
        for lo, hi in _chunks(n, (1000, 8192)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, (r, _, _) in zip(models, plan):
                m.feed(data[r, lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, [_snap(m) for m in models], st, what=(fmt, lo, hi), seen=seen)
        bank.close()
        got = [[e.word for e in m.events if not e.flags] for m in models]
        assert len(got[0]) >= 4 and set(got[0]) <= set(LEAD + list(PAYLOAD[0])) and len(got[1]) >= 4, got
        assert not set(got[2]) & set(PAYLOAD[0]) and not set(got[3]) & set(PAYLOAD[1])


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves word sync alone; a removed slot stops and keeps its arena; a slot set again starts
    cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 12
    x = _rows(Fs)
    n = x.shape[1]
    first = 3 * B + 5
    cut = 24000 + 7                                          # inside a word, behind the arena's second event
    bank = AleBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    for s, r in src.items():
        bank.set(s, ale_params(r))
    bank.set(2, ale_params(1))                               # for its increments; set again below, which is what counts
    models = [_model(bank, s) for s in range(4)]
    bank.remove(2)
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, [_snap(m) for m in models], st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, ale_params(1))
            src[2] = 1
            models[2] = _model(bank, 2, start=first)
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) >= 1
            assert int(st[0]["events"]) == 2 + int(st[0]["dropped"])
            assert int(st[0]["synced"]) == 1 and 0 < int(st[0]["wpos"]) < 49, "the cut must lie inside a word"
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
    _check(bank, [_snap(m) for m in models], st, slots=list(src))
    # set again: cold, the arena empty, zeros before it on the grid that went on
    bank.set(0, ale_params(0))
    assert int(bank.counts()[0]) == 0
    again = _model(bank, 0, start=n + cut)
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events and len(again.events) == 2
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = [_model(bank, s) for s in range(4)]
    src[0] = 0
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, [_snap(m) for m in fresh], st, slots=list(src))
    assert bank.events(1)[0].end_sample < n
    bank.close()


def test_word_sync_lost_and_regained(gpu):
    """three words, two words' time of tones drawn at random, four more words: the two are filed as holes, word sync ends
    at the second (lose = 2) and the words behind are found again by the search at every symbol"""
    Fs, B = 8000.0, 8
    words = [ale2g.word("TO", "ABC"), ale2g.word("TO", "ABC"), ale2g.word("TIS", "XYZ")]
    after = [ale2g.word("TO", "K1A"), ale2g.word("DATA", "BC@"), ale2g.word("TIS", "W1A"), ale2g.word("DATA", "W@@")]
    junk = np.random.default_rng(79).integers(0, 8, 2 * 49 + 5)      # and five symbols more: the grid of words moves
    sym = np.concatenate([ale2g.word_symbols(words), junk, ale2g.word_symbols(after)])
    x = ale2g.modulate_symbols(sym, Fs, amp=AMP, lead=30, tail=10)[None, :]
    bank = AleBank(Fs, B, 1, 8192)
    bank.set(0)
    model = _model(bank, 0)
    seen, synced = [0], []
    for lo, hi in _chunks(x.shape[1], (8192, 1000)):
        st = bank.process(x[:, lo:hi])
        model.feed(x[0, lo:hi])
        _check(bank, [_snap(model)], st, what=(lo, hi), seen=seen)
        synced.append(int(st[0]["synced"]))
    bank.close()
    ev = model.events
    flags = [e.flags for e in ev]
    print("ale sync", ale2g.read(ev), flags, synced)
    assert [e.word for e in ev[:3]] == words and flags[:5] == [0, 0, 0, 1, 1] and ev[3].err_a + ev[3].err_b >= 4
    assert [e.word for e in ev[5:]] == after and not any(flags[5:])
    assert ev[5].end_sample - ev[4].end_sample != 49 * 64         # the words behind are on another grid
    assert ale2g.read(ev)[-2:] == [("TO", "K1ABC"), ("TIS", "W1AW")]


# ---- loopback: an ALE USB station through a receiver bank's LINEAR channel, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """ALE audio from ale2g.modulate into a USB station; a receiver bank with a LINEAR channel of 300 to 2700 Hz at 48 kHz.
    The decode in place on the bank's stream must read the finished plane: status and events equal what the model makes of
    the same plane pulled to the host, and the call reads as sent, behind a scanning call that lets the receiver's gain
    and the decoder's levels settle."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    call = ale2g.individual_call("ABC", "XYZ12", scans=3)
    audio = ale2g.modulate(call, rate, amp=0.5, lead=20, tail=12)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=300.0, high=2700.0, second_lo=-f))
    ale = AleBank.beside(rx, max_slots=1, **ale2g.ale_config(rate))
    assert ale.samprate == rate and ale.max_samples == per_call * La and ale.block_len == 48
    ale.set(0, ale_params(0))
    assert ale.get_slot(0).W == 8
    model = _model(ale, 0)
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(ale.process_bank(rx))                                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = ale.events(0)
    pairs = ale2g.read(got)
    print("ale loopback:", pairs, [(e.err_a, e.err_b, e.split) for e in got])
    assert got == model.events
    assert pairs[-3:] == [("TO", "ABC"), ("TO", "ABC"), ("TIS", "XYZ12")], (pairs, got)
    for h in (mod, rx, ale):
        h.close()
