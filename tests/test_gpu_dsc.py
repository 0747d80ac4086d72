"""The DSC decoder bank (kq_dsc_*, ka9q_sdr_amd/csrc/kq_dsc.hip) on the GPU against the integer model of tests/dsc_model.py:
events (the symbols, nsym, flags, holes, from_rx, hole_mask, sync_sample, end_sample, sig, nse), arena counts and every
field of the status record -- the counters, the clock, the levels, the register, the open message with its 64 bytes, the
four window sums and the open frame's I and Q of both tones -- equal after every call, with no tolerance anywhere.  From
host and device memory, float and big-endian int16 input, padded rows, slots that share a row at different tone pairs,
calls of 1, B - 1, B, B + 1, 80, 4096 and 9000 samples, on 70 slots at (12000, 12) (18 workgroups of k_dsc, the last half
empty), at (12000, 8) with W = 15, at (39062.5, 32) with a fractional bit length, at (48000, 56) with several lanes to a
frame and at (96000, 8) with 1200 baud on 1300 / 2100 Hz; with a slot set in mid-frame, removed, set again and reset, an
arena of two events that fills, clear_events while a message is open, rows whose DX copies, RX copies, single symbols and
runs of symbols are knocked out so that the RX rescue, the holes, a failed check and the endings by rules (b) and (c) run
on the device, and in a loopback from a ModBank USB station through
a receiver bank's LINEAR channel.  The calls of one sample put a boundary between any two samples of some message, so its
five-place span crosses them all.  The model runs on the bank's own table, increments and bit length
(tests/test_dsc_args.py holds them equal to the model's), so nothing in the comparison is floating point but the
quantiser's one multiply.  The traffic is what tests/test_dsc_model.py shows the model to decode."""
import functools

import numpy as np
import pytest
import torch

import dsc_model as dm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import itu493
from ka9q_sdr_amd.dsc import STATUS_DTYPE, STATUS_WORDS, DscBank, dsc_params, status_array

pytestmark = pytest.mark.gpu

PAIRS = ((1785.0, 1615.0), (1615.0, 1785.0), (1085.0, 915.0))        # mark, space: an LSB channel's pair among them
VHF = ((1300.0, 2100.0),)


def _sizes(B):
    return (1, B - 1, B, B + 1, 80, 4096, 9000)


def _message(s):
    """slot s's traffic: a short individual call (17 symbols), every third with a category that differs"""
    return itu493.individual_call(200000000 + 1001 * s, 300000000 + 77 * s, category=100 + 2 * (s % 3), frequency=())


@functools.lru_cache(maxsize=None)
def _rows(Fs, B, S, baud, pairs):
    """row s: slot s's call at pair s's tones, amplitude 0.3, behind a lead-in of 8 bits plus s % B samples of silence;
    white noise at an Es/N0 of 20 dB.  ([S][n] float32, read-only)"""
    xs = []
    for s in range(S):
        mark, space = pairs[s % len(pairs)]
        x = itu493.modulate(itu493.bits(_message(s)), Fs, baud, mark, space, 0.3, lead=8 + (s % B) * baud / Fs, tail=6)
        xs.append(x)
    n = max(len(x) for x in xs)
    out = np.zeros((S, n), np.float32)
    for s, x in enumerate(xs):
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(300 + s).normal(0.0, dm.noise_sigma(0.3, 20.0, Fs, baud), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _models(bank, S, **kw):
    """a model per slot on the bank's own table, increments and bit length"""
    table, out = bank.get_table(), []
    for s in range(S):
        g = bank.get_slot(s)
        out.append(dm.DscModel(bank.samprate, bank.block_len, table=table, incs=(g.inc_m, g.inc_s), tb=g.tb, warm=bank.warm,
                               snr=bank.snr, min_p=bank.min_p, acq=bank.acq, lose=bank.lose, input_scale=bank.input_scale,
                               max_events=bank.max_events, **kw))
        assert out[-1].W == g.W
    return out


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


PARITY = [(12000.0, 12, 70, 100.0, PAIRS), (12000.0, 8, 3, 100.0, PAIRS), (39062.5, 32, 3, 100.0, PAIRS),
          (48000.0, 56, 3, 100.0, PAIRS), (96000.0, 8, 3, 1200.0, VHF)]


@pytest.mark.parametrize("Fs,B,S,baud,pairs", PARITY, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_parity_from_host_and_device_memory(gpu, Fs, B, S, baud, pairs):
    x = _rows(Fs, B, S, baud, pairs)
    n = x.shape[1]
    cuts = _chunks(n, _sizes(B))
    want = None
    for device in (False, True):
        bank = DscBank(Fs, B, S, 9000)
        for s in range(S):
            mark, space = pairs[s % len(pairs)]
            bank.set(s, dsc_params(source=s, mark=mark, space=space, baud=baud))
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, S), []
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
    print("dsc parity", Fs, B, S, [(m.W, m.tb, len(m.events), m.syncs) for m in models[:3]])
    # 20 dB: every slot files the call it was sent, whole, and none is read through its RX copies
    for s, m in enumerate(models):
        assert len(m.events) == 1, (s, m.events)
        e = m.events[0]
        assert (e.flags, e.holes, e.from_rx) == (0, 0, 0) and list(e.sym[:e.nsym]) == _message(s), (s, e)
        assert itu493.read(m.events)[0]["to"] == "%09d" % (200000000 + 1001 * s)


def _knock(bits, places, dots=20):
    """the bits with the first bit of every place named turned over: one wrong bit, which the symbol code always sees"""
    out = np.array(bits, np.uint8)
    for p in places:
        out[dots + 10 * p] ^= 1
    return out


def _both(i):
    """the DX and the RX place of message symbol i"""
    return (12 + 2 * i, 17 + 2 * i)


@functools.lru_cache(maxsize=None)
def _damaged():
    """the tracker's paths above the bit that clean traffic never takes, a row each: (name, bits, what the model must make
    of it).  LONG is 66 symbols with no end of sequence among the first 64 and both copies of symbols 40 and 50 gone"""
    call = itu493.individual_call(232001234, 211239870)
    n = len(call)
    b = itu493.bits(call)
    wrong = itu493.sequence(call)
    wrong[12 + 2 * 4] = wrong[17 + 2 * 4] = call[4] ^ 3
    long_ = [itu493.INDIVIDUAL] * 2 + list(range(62)) + [1, 2]
    lose = [p for i in (10, 11, 12) for p in _both(i)]
    early = [p for i in (3, 4, 5) for p in _both(i)]
    return (
        ("dx gone", _knock(b, range(12, 12 + 2 * n, 2)), dict(events=1, flags=0, holes=0, from_rx=n, nsym=n)),
        ("rx gone", _knock(b, range(17, 17 + 2 * n, 2)), dict(events=1, flags=0, holes=0, from_rx=0, nsym=n)),
        ("one hole", _knock(b, _both(9)), dict(events=1, flags=itu493.CHECK, holes=1, hole_mask=1 << 9, nsym=n)),
        ("check gone", _knock(b, _both(n - 1)), dict(events=1, flags=itu493.CHECK, holes=1, hole_mask=1 << (n - 1), nsym=n)),
        ("wrong symbol", itu493.place_bits(wrong), dict(events=1, flags=itu493.CHECK, holes=0, from_rx=0, nsym=n)),
        ("lost", _knock(b, lose), dict(events=1, flags=itu493.LOST | itu493.CHECK, holes=3, hole_mask=7 << 10, nsym=13, aborted=0)),
        ("aborted", _knock(b, early), dict(events=0, aborted=1)),
        ("truncated", _knock(itu493.bits(long_), _both(40) + _both(50)),
         dict(events=1, flags=itu493.TRUNCATED | itu493.CHECK, holes=2, hole_mask=1 << 40 | 1 << 50, nsym=64)),
    )


def test_diversity_and_message_endings(gpu):
    """What is new above the bit, on the device: a message read through its RX copies alone and through its DX copies
    alone; both copies of one symbol gone (a hole, 0xFF in the message, its bit in hole_mask) and of the error-check symbol;
    a wrong symbol in both copies, which only the check sees; rule (c) after at least eight resolved symbols (filed, lost)
    and after fewer (counted in aborted); rule (b) at 64 symbols, with holes at symbols 40 and 50, beyond the low word of
    hole_mask.  Status and events equal the model's after every call, from host and from device memory; and the model makes
    of every row what the row was built to show"""
    Fs, B = 12000.0, 12
    rows = _damaged()
    xs = [itu493.modulate(bits, Fs, amp=0.3, lead=8 + s / Fs, tail=6) for s, (_, bits, _) in enumerate(rows)]
    n = max(len(x) for x in xs)
    x = np.zeros((len(rows), n), np.float32)
    for s, v in enumerate(xs):
        x[s, :len(v)] = v
        x[s] += np.random.default_rng(400 + s).normal(0.0, dm.noise_sigma(0.3, 20.0, Fs), n).astype(np.float32)
    S = len(rows)
    cuts = _chunks(n, _sizes(B))
    want = None
    for device in (False, True):
        bank = DscBank(Fs, B, S, 9000)
        for s in range(S):
            bank.set(s, dsc_params(source=s))
        if want is None:
            models, want = _models(bank, S), []
            for a, b in cuts:
                for s, m in enumerate(models):
                    m.feed(x[s, a:b])
                want.append(_snap(models))
        st_t, seen = _plane(bank), [0] * S
        for (a, b), w in zip(cuts, want):
            st = _device_call(bank, x[:, a:b], 1, st_t) if device else bank.process(x[:, a:b])
            _check(bank, w, st, what=(device, a, b), seen=seen)
        bank.close()
    for (name, _, must), m in zip(rows, models):
        got = dict(events=len(m.events), aborted=m.aborted)
        if m.events:
            got.update({k: getattr(m.events[0], k) for k in ("flags", "holes", "from_rx", "hole_mask", "nsym")})
        assert m.syncs == 1 and not m.synced and all(got[k] == v for k, v in must.items()), (name, got, must)
    by = {name: m for (name, _, _), m in zip(rows, models)}
    assert by["one hole"].events[0].sym[9] == itu493.HOLE and itu493.read(by["one hole"].events)[0]["ok"]
    assert by["wrong symbol"].events[0].sym[4] == itu493.individual_call(232001234, 211239870)[4] ^ 3
    assert by["truncated"].events[0].sym[40] == by["truncated"].events[0].sym[50] == itu493.HOLE


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range.  Row 0 carries two
    stations, at 1785 / 1615 Hz and at 1085 / 915 Hz; slots 0, 1, 3 and 4 read it at those pairs, at the first pair turned
    over (the call comes out marked inverted) and at 4500 / 4330 Hz, where there is only what the other two splatter; slot 2
    reads row 1."""
    Fs, B = 12000.0, 12
    a = itu493.modulate(itu493.bits(_message(0)), Fs, amp=0.3, lead=10, tail=6)
    b = itu493.modulate(itu493.bits(_message(1)), Fs, mark=1085.0, space=915.0, amp=0.2, lead=25, tail=6)
    n = max(len(a), len(b))
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] += a
    x[0, :len(b)] += b
    r1 = _rows(Fs, B, 2, 100.0, PAIRS)[1]
    x[1, :min(n, len(r1))] = r1[:n]
    x += np.random.default_rng(5).normal(0.0, 0.02, x.shape).astype(np.float32)
    loud = x * np.float32(4.0)                               # clips: (0.3 + 0.2) x 4
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = dm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    plan = [(1785.0, 1615.0), (1085.0, 915.0), (1615.0, 1785.0), (1615.0, 1785.0), (4500.0, 4330.0)]
    src = (0, 0, 1, 0, 0)
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = DscBank(Fs, B, 5, 8192)
        for s, ((mark, space), r) in enumerate(zip(plan, src)):
            bank.set(s, source=r, mark=mark, space=space)
        models = _models(bank, 5)
        st_t, seen = _plane(bank), [0] * 5
        for lo, hi in _chunks(n, (1000, 8192)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, r in zip(models, src):
                m.feed(data[r, lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, lo, hi), seen=seen)
        bank.close()
    got = [itu493.read(m.events) for m in models]            # the int16 pass: the words -32768 do no harm
    assert [len(g) for g in got] == [1, 1, 1, 1, 0], got
    assert got[0][0]["symbols"] == _message(0) and got[1][0]["symbols"] == _message(1) and got[2][0]["symbols"] == _message(1)
    assert got[3][0]["symbols"] == _message(0) and got[3][0]["inverted"] and not got[0][0]["inverted"] and not got[2][0]["inverted"]


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves the open message alone; a removed slot stops and keeps its arena; a slot set again
    starts cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 12
    one = _rows(Fs, B, 2, 100.0, PAIRS)
    x = np.concatenate([one, one, one, one], axis=1)         # four calls in a row on each
    n1, n = one.shape[1], 4 * one.shape[1]
    first = 3 * B + 7
    bank = DscBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    plan = [PAIRS[0], PAIRS[1], PAIRS[1], PAIRS[0]]
    for s in range(4):
        bank.set(s, dsc_params(src.get(s, 1), *plan[s]))     # (slot 2 for its increments; set again below, which is what counts)
    models = _models(bank, 4)
    bank.remove(2)
    cut = 3 * n1 + n1 // 2                                   # inside the fourth call
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, dsc_params(1, *plan[2]))
            src[2] = 1
            models[2] = _models(bank, 4, start=first)[2]
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) == 1 and int(st[0]["events"]) == 3
            assert int(st[0]["synced"]) == 1 and 0 < int(st[0]["nsym"]) < 17, "the cut must lie inside a message for what follows to mean anything"
            bank.clear_events()
            for m in models:
                m.clear_events()
            assert not bank.counts().any()
    assert int(st[0]["dropped"]) == 1 and int(st[0]["events"]) == 4 and int(bank.counts()[0]) == 1
    assert bank.events(0) == bank.events(3) and bank.events(0)[0].sym[:17] == bytes(_message(0))
    assert int(st[2]["frames"]) == int(st[1]["frames"]) - 3 and int(st[2]["frames"]) == (n - 3 * B) // B
    # a removed slot stops: nothing is written for it, its arena stays; the others go on
    bank.remove(0)
    kept = bank.events(0)
    del src[0]
    st = bank.process(x[:, :cut])
    for s, r in src.items():
        models[s].feed(x[r, :cut])
    assert not st[0].tobytes().strip(b"\0") and bank.events(0) == kept and len(kept) == 1
    _check(bank, _snap(models), st, slots=list(src))
    # set again: cold, the arena empty, zeros before it on the grid that went on
    bank.set(0, dsc_params(0, *plan[0]))
    assert int(bank.counts()[0]) == 0
    again = _models(bank, 4, start=n + cut)[0]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events and len(again.events) == 2
    assert again.dropped == 1
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, 4)
    src[0] = 0
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, slots=list(src))
    assert bank.events(1)[0].end_sample < n1
    bank.close()


# ---- loopback: an FSK-keyed USB station through a receiver bank's LINEAR channel, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """DSC audio from itu493.modulate (100 baud, 1785 / 1615 Hz) into a USB station; a receiver bank with a LINEAR channel of
    1400 to 2000 Hz at 48 kHz.  The decode in place on the bank's stream must read the finished plane: status and events
    equal what the model makes of the same plane pulled to the host, and the parsed message is the one sent."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    B = itu493.dsc_config(rate)["block_len"]
    assert B == 48
    sent = itu493.distress_alert(211239870, position="0521301234", time="1359")
    lead_in = np.ones(60, np.uint8)                          # a steady tone that lets the receiver's gain settle
    audio = itu493.modulate(np.concatenate([lead_in, itu493.bits(sent)]), rate, amp=0.5, lead=10, tail=20)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=1400.0, high=2000.0, second_lo=-f))
    dsc = DscBank.beside(rx, B, 1)
    assert dsc.samprate == rate and dsc.max_samples == per_call * La
    dsc.set(0, dsc_params(0))
    assert dsc.get_slot(0).W == 10
    model = _models(dsc, 1)[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(dsc.process_bank(rx))                                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = dsc.events(0)
    msgs = itu493.read(got)
    print("dsc loopback:", msgs, _status(st[0]))
    assert got == model.events and len(got) == 1
    assert msgs[0]["ok"] and msgs[0]["symbols"] == sent and msgs[0]["kind"] == "distress"
    assert (msgs[0]["frm"], msgs[0]["position"], msgs[0]["time"]) == ("211239870", "0521301234", "1359")
    for h in (mod, rx, dsc):
        h.close()
