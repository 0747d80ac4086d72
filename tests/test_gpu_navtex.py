"""The NAVTEX decoder bank (kq_navtex_*, ka9q_sdr_amd/csrc/kq_navtex.hip) on the GPU against the integer model of
tests/navtex_model.py: events (code, flags, dx, rx, end_sample, sig, nse), arena counts and every field of the status
record -- the counters, the clock, the levels, the 128-bit register, the place, the run, the four window sums and the open
frame's I and Q of both tones -- equal after every call, with no tolerance anywhere.  From host and device memory, float
and big-endian int16 input, padded rows, slots that share a row at different tone pairs, calls of 1, B - 1, B, B + 1, 80, 4096
and 9000 samples, on 70 slots at (12000, 12) (18 workgroups of k_navtex, the last half empty), at (12000, 8) with W = 15, at
(39062.5, 32) with a fractional bit length and at (48000, 56) with several lanes to a frame; with a slot set in mid-frame,
removed, set again and reset, an arena of two events that fills, clear_events while in sync, rows whose DX copies, RX copies
and single characters are knocked out, a fade that drops sync with the phasing behind it, a stream entered in mid-message,
and in a loopback from a ModBank USB station through a receiver bank's LINEAR channel.  The calls of one sample put a
boundary between any two samples of some character's 35-bit span.  The model runs on the bank's own table, increments and
bit length (tests/test_navtex_args.py holds them equal to the model's), so nothing in the comparison is floating point but
the quantiser's one multiply.  The traffic is what tests/test_navtex_model.py shows the model to decode."""
import functools

import numpy as np
import pytest
import torch

import navtex_model as nm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import ccir476 as cc
from ka9q_sdr_amd.navtex import STATUS_DTYPE, STATUS_WORDS, NavtexBank, navtex_params, status_array

pytestmark = pytest.mark.gpu

PAIRS = ((1785.0, 1615.0), (1615.0, 1785.0), (1085.0, 915.0))        # mark, space: an LSB channel's pair among them
LINES = ("GALE NW 7", "FOG 1/2 NM", "ICE: NIL")


def _sizes(B):
    return (1, B - 1, B, B + 1, 80, 4096, 9000)


def _text(s):
    """slot s's traffic: about 20 characters, the serial number by slot"""
    return "ZCZC FA%02d\r\n%s\r\nNNNN" % (s % 100, LINES[s % 3])


@functools.lru_cache(maxsize=None)
def _rows(Fs, B, S, pairs=PAIRS):
    """row s: slot s's message behind 8 phasing pairs at pair s's tones, amplitude 0.3, behind a lead-in of 8 bits plus
    s % B samples of silence; white noise at an Es/N0 of 20 dB.  ([S][n] float32, read-only)"""
    xs = []
    for s in range(S):
        mark, space = pairs[s % len(pairs)]
        b = cc.bits(cc.places(cc.codes_of(_text(s)), phasing=(8, 2)))
        xs.append(cc.modulate(b, Fs, cc.BAUD, mark, space, 0.3, lead=8 + (s % B) * cc.BAUD / Fs, tail=6))
    n = max(len(x) for x in xs)
    out = np.zeros((S, n), np.float32)
    for s, x in enumerate(xs):
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(300 + s).normal(0.0, nm.noise_sigma(0.3, 20.0, Fs), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _models(bank, S, **kw):
    """a model per slot on the bank's own table, increments and bit length"""
    table, out = bank.get_table(), []
    for s in range(S):
        g = bank.get_slot(s)
        out.append(nm.NavtexModel(bank.samprate, bank.block_len, table=table, incs=(g.inc_m, g.inc_s), tb=g.tb, warm=bank.warm,
                                  snr=bank.snr, min_p=bank.min_p, acq=bank.acq, pairs=bank.pairs, lose=bank.lose,
                                  input_scale=bank.input_scale, max_events=bank.max_events, **kw))
        assert out[-1].W == g.W
    return out


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


def _sent(m, n):
    """the model's first n events as text, which must be clean"""
    assert all(e.flags & ~cc.INVERTED == 0 for e in m.events[:n]), m.events[:n]
    return cc.read_text(m.events[:n])


def _both_ways(x, S, setup, cuts, **kw):
    """the rows through a bank from host memory and from device memory, held against the models after every call; returns
    the models"""
    Fs, B = kw.pop("geometry")
    want = None
    for device in (False, True):
        bank = NavtexBank(Fs, B, S, 9000, **kw)
        setup(bank)
        if want is None:                                         # the models' records after every call, made once
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
    return models


PARITY = [(12000.0, 12, 70), (12000.0, 8, 3), (39062.5, 32, 3), (48000.0, 56, 3)]


@pytest.mark.parametrize("Fs,B,S", PARITY)
def test_parity_from_host_and_device_memory(gpu, Fs, B, S):
    x = _rows(Fs, B, S)
    n = x.shape[1]

    def setup(bank):
        for s in range(S):
            mark, space = PAIRS[s % len(PAIRS)]
            bank.set(s, navtex_params(source=s, mark=mark, space=space))

    models = _both_ways(x, S, setup, _chunks(n, _sizes(B)), geometry=(Fs, B))
    assert all(m.frames == n // B for m in models)
    print("navtex parity", Fs, B, S, [(m.W, m.tb, len(m.events), m.syncs) for m in models[:3]])
    # 20 dB: every slot reads the text it was sent, every character a clean pair
    for s, m in enumerate(models):
        k = len(cc.codes_of(_text(s)))
        assert m.syncs == 1 and m.tsyncs == 0 and _sent(m, k) == _text(s), (s, m.events)
        assert cc.messages(cc.read_text(m.events[:k])) == [cc.Message("F", "A", "%02d" % s, LINES[s % 3], True)]


def _damage(p, where, word=0x7F):
    out = list(p)
    for k in where:
        out[k] = word
    return out


@functools.lru_cache(maxsize=None)
def _paths():
    """the tracker's paths above the bit that clean traffic never takes, a row each: (name, bits, lead in bits)"""
    a = 8
    short = cc.codes_of("ZCZC FA01")                             # eleven codes: a copy gone on every one stays below `lose`
    p = cc.places(short, phasing=(a, 3))
    n = len(short)
    codes = cc.codes_of(_text(0))
    q = cc.places(codes, phasing=(a, 3))
    other = cc.CODE["Q"] if codes[12] != cc.CODE["Q"] else cc.CODE["X"]
    second = cc.places(cc.codes_of("ZCZC GB17\r\nNIL\r\nNNNN"), phasing=(10, 3))
    faded = _damage(cc.places(codes, phasing=(a, 0)), range(2 * a + 20, 2 * a + 2 * len(codes) + 6)) + second
    long_ = cc.codes_of("ZCZC FA01\r\nGALE WARNING FORTIES NW 7/8 BACKING W-LY 5.\r\nNNNN")
    late = cc.places(long_, phasing=(0, 3))[2 * 20:]             # entered at character 20's DX place: no phasing in sight
    return (("dx gone", cc.bits(_damage(p, [2 * a + 2 * i for i in range(n)])), 8),
            ("rx gone", cc.bits(_damage(p, [2 * a + 2 * i + 5 for i in range(n)])), 8),
            ("unresolved", cc.bits(_damage(q, [2 * a + 18, 2 * a + 18 + 5])), 8),
            ("differ", cc.bits(_damage(q, [2 * a + 2 * 12 + 5], other)), 8),
            ("loss and resync", cc.bits(faded), 8),
            ("mid-stream", cc.bits(late), 8))


def test_diversity_loss_and_traffic_sync(gpu):
    """What is new above the bit, on the device, a row each: a message read through its RX copies alone and through its DX
    copies alone; both copies of one character gone (0x7F, flag bit 0); another character in the RX copy (flag bit 2, the
    DX copy taken); a fade that outlasts `lose` and drops sync, and the phasing behind it that takes it again; a stream
    entered in mid-message that takes sync on the traffic.  Status and events equal the model's after every call, from host
    and from device memory; and the model makes of every row what the row was built to show"""
    Fs, B = 12000.0, 12
    rows = _paths()
    xs = [cc.modulate(bits, Fs, amp=0.3, lead=lead + s / Fs, tail=6) for s, (_, bits, lead) in enumerate(rows)]
    n = max(len(x) for x in xs)
    S = len(rows)
    x = np.zeros((S, n), np.float32)
    for s, v in enumerate(xs):
        x[s, :len(v)] = v
        x[s] += np.random.default_rng(400 + s).normal(0.0, nm.noise_sigma(0.3, 20.0, Fs), n).astype(np.float32)

    def setup(bank):
        for s in range(S):
            bank.set(s, navtex_params(source=s))

    models = _both_ways(x, S, setup, _chunks(n, _sizes(B)), geometry=(Fs, B))
    by = {name: m for (name, _, _), m in zip(rows, models)}
    short, codes = cc.codes_of("ZCZC FA01"), cc.codes_of(_text(0))
    k = len(short)
    m = by["dx gone"]
    assert [e.code for e in m.events[:k]] == short and all(e.flags == cc.FROM_RX for e in m.events[:k]) and m.syncs == 1
    m = by["rx gone"]
    assert [e.code for e in m.events[:k]] == short and all(e.flags == 0 and not nm.is_char(e.rx) for e in m.events[:k])
    m = by["unresolved"]
    assert (m.events[9].code, m.events[9].flags) == (cc.NONE, cc.UNRESOLVED) and cc.read_text(m.events[:len(codes)]).count("*") == 1
    assert [e.code for i, e in enumerate(m.events[:len(codes)]) if i != 9] == codes[:9] + codes[10:]
    m = by["differ"]
    assert (m.events[12].code, m.events[12].flags, m.events[12].dx) == (codes[12], cc.DIFFER, codes[12])
    assert m.events[12].rx != codes[12] and [e.code for e in m.events[:len(codes)]] == codes
    m = by["loss and resync"]
    assert (m.syncs, m.losses, m.tsyncs) == (2, 1, 0)
    assert cc.messages(cc.read_text(m.events))[-1] == cc.Message("G", "B", "17", "NIL", True)
    m = by["mid-stream"]
    long_ = cc.codes_of("ZCZC FA01\r\nGALE WARNING FORTIES NW 7/8 BACKING W-LY 5.\r\nNNNN")
    # (the cold clock settles during the first place, whose copy is lost: one character more than `pairs` behind the entry)
    assert (m.syncs, m.tsyncs) == (0, 1) and [e.code for e in m.events[:len(long_) - 25]] == long_[25:]
    assert all(e.flags == 0 for e in m.events[:len(long_) - 25])


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_shared_rows_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range.  Row 0 carries two
    stations, at 1785 / 1615 Hz and at 1085 / 915 Hz; slots 0, 1, 3 and 4 read it at those pairs, at the first pair turned
    over (the text comes out marked inverted) and at 4500 / 4330 Hz, where there is only what the other two splatter; slot 2
    reads row 1."""
    Fs, B = 12000.0, 12
    a = cc.modulate(cc.bits(cc.places(cc.codes_of(_text(0)), phasing=(8, 2))), Fs, amp=0.3, lead=10, tail=6)
    b = cc.modulate(cc.bits(cc.places(cc.codes_of(_text(1)), phasing=(8, 2))), Fs, mark=1085.0, space=915.0, amp=0.2, lead=25, tail=6)
    n = max(len(a), len(b))
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] += a
    x[0, :len(b)] += b
    r1 = _rows(Fs, B, 2)[1]
    x[1, :min(n, len(r1))] = r1[:n]
    x += np.random.default_rng(5).normal(0.0, 0.02, x.shape).astype(np.float32)
    loud = x * np.float32(4.0)                               # clips: (0.3 + 0.2) x 4
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.02
    words = nm.fm.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:100:7] = -32768
    words[0, -3:] = -32768
    plan = [(1785.0, 1615.0), (1085.0, 915.0), (1615.0, 1785.0), (1615.0, 1785.0), (4500.0, 4330.0)]
    src = (0, 0, 1, 0, 0)
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = NavtexBank(Fs, B, 5, 8192)
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
    k0, k1 = len(cc.codes_of(_text(0))), len(cc.codes_of(_text(1)))       # the int16 pass: the words -32768 do no harm
    assert _sent(models[0], k0) == _text(0) and _sent(models[1], k1) == _text(1) and _sent(models[2], k1) == _text(1)
    assert _sent(models[3], k0) == _text(0) and all(e.flags == cc.INVERTED for e in models[3].events[:k0])
    assert models[3].inverted == 1 and models[0].inverted == 0 and models[2].inverted == 0
    assert models[4].syncs == 0 and models[4].tsyncs == 0 and not models[4].events


def test_slot_lifecycle(gpu):
    """Slot 2 is set inside frame 3 and sees zeros before it; an arena of two events fills and counts what it drops;
    clear_events empties it and leaves the sync alone; a removed slot stops and keeps its arena; a slot set again starts
    cold with an empty arena; reset starts the grid over"""
    Fs, B = 12000.0, 12
    one = _rows(Fs, B, 2)
    x = np.concatenate([one, one], axis=1)                   # the message twice on each row
    n1, n = one.shape[1], 2 * one.shape[1]
    first = 3 * B + 7
    bank = NavtexBank(Fs, B, 4, n, max_events=2)
    src = {0: 0, 1: 1, 3: 0}
    plan = [PAIRS[0], PAIRS[1], PAIRS[1], PAIRS[0]]
    for s in range(4):
        bank.set(s, navtex_params(src.get(s, 1), *plan[s]))  # (slot 2 for its increments; set again below, which is what counts)
    models = _models(bank, 4)
    bank.remove(2)
    cut = n1 // 2                                            # inside the first message
    for a, b in ((0, first), (first, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, navtex_params(1, *plan[2]))
            src[2] = 1
            models[2] = _models(bank, 4, start=first)[2]
        if b == cut:
            assert int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) >= 1 and int(st[0]["events"]) == 2 + int(st[0]["dropped"])
            assert int(st[0]["synced"]) == 1, "the cut must lie inside a message for what follows to mean anything"
            bank.clear_events()
            for m in models:
                m.clear_events()
            assert not bank.counts().any()
    assert int(st[0]["synced"]) in (0, 1) and int(bank.counts()[0]) == 2 and int(st[0]["dropped"]) > 2
    assert bank.events(0) == bank.events(3) == models[0].events
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
    bank.set(0, navtex_params(0, *plan[0]))
    assert int(bank.counts()[0]) == 0
    again = _models(bank, 4, start=n + cut)[0]
    st = bank.process(x[:, :cut])
    again.feed(x[0, :cut])
    assert _status(st[0]) == again.status() and bank.events(0) == again.events and len(again.events) == 2
    assert again.dropped >= 1 and again.syncs == 1
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
    """NAVTEX audio from ccir476.modulate (100 baud, 1785 / 1615 Hz) into a USB station; a receiver bank with a LINEAR
    channel of 1400 to 2000 Hz at 48 kHz.  The decode in place on the bank's stream must read the finished plane: status
    and events equal what the model makes of the same plane pulled to the host, and the message is the one sent."""
    per_call = 64
    rate = FS // INTERP
    La = LB // INTERP
    B = cc.navtex_config(rate)["block_len"]
    assert B == 48
    text = "ZCZC FA01\r\nGALE NW 7\r\nNNNN"
    codes = cc.codes_of(text)
    lead_in = np.ones(60, np.uint8)                          # a steady tone that lets the receiver's gain settle
    audio = cc.modulate(np.concatenate([lead_in, cc.bits(cc.places(codes, phasing=(8, 3)))]), rate, amp=0.5, lead=10, tail=20)
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio), np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=1400.0, high=2000.0, second_lo=-f))
    nav = NavtexBank.beside(rx, B, 1)
    assert nav.samprate == rate and nav.max_samples == per_call * La
    nav.set(0, navtex_params(0))
    assert nav.get_slot(0).W == 10
    model = _models(nav, 1)[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(nav.process_bank(rx))                                   # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = nav.events(0)
    read = cc.read_text(got[:len(codes)])
    print("navtex loopback:", repr(cc.read_text(got)), _status(st[0]))
    assert got == model.events and len(got) >= len(codes)
    assert read == text and cc.messages(read) == [cc.Message("F", "A", "01", "GALE NW 7", True)]
    for h in (mod, rx, nav):
        h.close()
