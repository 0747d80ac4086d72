"""The SAME decoder bank (kq_same_*, ka9q_sdr_amd/csrc/kq_same.hip) on the GPU against the integer model of
tests/same_model.py: events (code, flags, index, errs, end_sample, sig, nse), arena counts and every field of the status
record -- the counters, the clock, the levels, the register, the byte and its run, the four window sums and the open
frame's I and Q of both tones -- equal after every call, with no tolerance anywhere.  The input is one alert with a
one-location header, three bursts a second apart, some 4.7 s at 48 kHz, on four rows with a delay and noise of their own.
The whole stream in one call; random cuts of 1 to 4096 samples with cuts inside a frame and calls of one sample; calls so
short that the host takes every number of lanes to a frame from 1 to 64; host float, host big-endian int16 and device
input with padded rows; slots that share a row, one of them with the tones exchanged, which must file nothing; a slot set
in the middle of a burst, removed, and the bank reset; an arena of eight events that fills; clear_events between the
bursts; 16384 slots for one burst; the whole alert with its attention signal and its three ends of message; and rows
built bit by bit for what a clean alert never does -- wrong bits in the sync, bad bytes, an end by `lose` and one by
max_len; and a loopback from a ModBank USB station through a receiver bank's LINEAR channel, decoded in place.  The model runs on the bank's own table, increments and bit length
(tests/test_same_args.py holds them equal to the model's), so nothing in the comparison is floating point but the
quantiser's one multiply.  The traffic is what tests/test_same_model.py shows the model to decode."""
import functools

import numpy as np
import pytest

import same_model as sm
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import eas
from ka9q_sdr_amd.same import STATUS_DTYPE, STATUS_WORDS, SameBank, same_params, status_array

on_gpu = pytest.mark.gpu                                          # (not the file's mark: the reference's own check needs no GPU)

FS, B, ROWS = 48000.0, 8, 4
PREAMBLE = eas.PREAMBLE_BYTES
TEXT = eas.header("WXR", "RWT", [12345], "0015", "1231200", "KABC/FM")


@functools.lru_cache(maxsize=None)
def _rows(Fs=FS, repeats=3, rows=ROWS):
    """row s: the alert's header bursts, amplitude 0.3, behind 50 ms and s * 2.3 samples of silence (so that the bit edges
    fall elsewhere between the samples and in the frames on every row); white noise at an Es/N0 of 20 dB.  ([rows][n]
    float32, read-only)"""
    xs = [eas.modulate(TEXT, Fs, eom=False, repeats=repeats, amp=0.3, lead=0.05 + s * 2.3 / Fs, tail=0.05) for s in range(rows)]
    n = max(len(x) for x in xs)
    out = np.zeros((rows, n), np.float32)
    for s, x in enumerate(xs):
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(500 + s).normal(0.0, sm.noise_sigma(0.3, 20.0, Fs), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _model(bank, slot, **kw):
    """a model of the slot on the bank's own table, increments and bit length"""
    g = bank.get_slot(slot)
    m = sm.SameModel(bank.samprate, bank.block_len, table=bank.get_table(), incs=(g.inc_m, g.inc_s), tb=g.tb, warm=bank.warm,
                     snr=bank.snr, min_p=bank.min_p, sync_errs=bank.sync_errs, lose=bank.lose, max_len=bank.max_len,
                     input_scale=bank.input_scale, max_events=bank.max_events, **kw)
    assert m.W == g.W
    return m


def _models(bank, S, **kw):
    return [_model(bank, s, **kw) for s in range(S)]


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "events"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "event")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


@functools.lru_cache(maxsize=None)
def _whole():
    """the reference made once: what the model makes of each row of _rows() in one piece, as (status, events)"""
    x = _rows()
    out = []
    for s in range(ROWS):
        m = sm.SameModel(FS, B).feed(x[s])
        out.append((m.status(), tuple(m.events)))
    return tuple(out)


def _read_whole(events):
    """three header bursts, each the text sent and ended by the grammar"""
    bursts = eas.read(events)
    assert [(b.kind, b.text, b.reason, b.bad) for b in bursts] == [("Z", TEXT, eas.COMPLETE, [])] * 3, bursts
    assert [a.text for a in eas.vote(bursts, FS)] == [TEXT]


def _run(x, bank, models, src, cuts, device=False, fmt=kq.KQ_PCM_F32, s16=False, seen=None):
    """the cuts through the bank and the models (slot s reads row src[s]); everything is held equal after every call"""
    st_t = _plane(bank) if device else None
    seen = [0] * len(models) if seen is None else seen
    for a, b in cuts:
        if device:
            nblocks = 4 if (b - a) % 4 == 0 else 1
            st = _device_call(bank, x[:, a:b], nblocks, st_t, fmt)
        else:
            st = bank.process(x[:, a:b], 2 if (b - a) % 2 == 0 else 1, fmt)
        for m, r in zip(models, src):
            m.feed(x[r, a:b], s16=s16)
        _check(bank, _snap(models), st, what=(device, fmt, a, b), seen=seen)
    return st


def _bank(S, n, **kw):
    """slot s on row s"""
    bank = SameBank(FS, B, S, n, **kw)
    for s in range(S):
        bank.set(s, same_params(source=s))
    return bank


def _random_cuts(n, seed):
    """block lengths 1..4096, most of them no multiple of the frame, with runs of single samples strewn in"""
    rng = np.random.default_rng(seed)
    at, out = 0, []
    while at < n:
        for m in ([1] * 9 if rng.integers(0, 8) == 0 else [int(rng.integers(1, 4097))]):
            m = min(m, n - at)
            if m:
                out.append((at, at + m))
                at += m
    return out


def test_the_model_reads_the_rows():
    """no GPU work, and no `gpu` mark: what the cases below compare against is a decode of the alert, and of the damaged
    rows every path the clean alert never takes"""
    for status, events in _whole():
        _read_whole(events)
        assert (status["syncs"], status["complete"], status["lost"], status["truncated"], status["dropped"]) == (3, 3, 0, 0, 0)
    _damaged_paths([sm.SameModel(FS, B, **DAMAGED_BANK).feed(x) for x in _damaged()])


DAMAGED_BANK = dict(sync_errs=4, lose=2, max_len=16)


@functools.lru_cache(maxsize=None)
def _damaged():
    """three rows built bit by bit, for a bank with sync_errs = 4, lose = 2 and max_len = 16.  Row 0: a header burst with three
    of its 48 sync bits wrong, which runs into max_len.  Row 1: one with bit 7 set in byte 2 and in bytes 5 and 6 behind ZCZC: a
    bad byte alone, then two in a row.  Row 2: an end of message with two of its sync bits wrong, then a whole header
    burst.  Noise at 20 dB.  ([3][n] float32, read-only)"""
    at = 8 * PREAMBLE + 32 - 48                                    # the first of the 48 sync bits
    one, two, eom = eas.burst(TEXT), eas.burst(TEXT), eas.burst(eas.EOM)
    one[[at + 1, at + 8, at + 38]] ^= 1
    two[[8 * (PREAMBLE + 4 + k) + 7 for k in (2, 5, 6)]] ^= 1
    eom[[at + 3, at + 44]] ^= 1
    rows = []
    for s, bursts in enumerate(([one], [two], [eom, eas.burst(TEXT)])):
        parts, t = [], 0.05 * FS + 2.3 * s
        for b in bursts:
            parts.append(eas.afsk(b, FS, t, amp=0.3))
            t += len(b) * FS / eas.BAUD + 0.2 * FS
        x = np.zeros(int(t), np.float64)
        for n0, v in parts:
            x[n0:n0 + len(v)] += v
        rows.append(x)
    n = max(len(x) for x in rows)
    out = np.zeros((len(rows), n), np.float32)
    for s, x in enumerate(rows):
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(600 + s).normal(0.0, sm.noise_sigma(0.3, 20.0, FS), n).astype(np.float32)
    out.setflags(write=False)
    return out


def _damaged_paths(models):
    """the models of _damaged()'s rows took every path they were built for"""
    got = [[(b.kind, b.text, b.bad, b.reason, b.errs) for b in eas.read(m.events)] for m in models]
    cut = TEXT[:4 + 16]
    assert got[0] == [("Z", cut, [], eas.LENGTH, 3)], got[0]
    assert got[1] == [("Z", "ZCZC-W?R-??", [6, 9, 10], eas.LOST, 0)], got[1]
    assert got[2] == [("N", "NNNN", [], 0, 2), ("Z", cut, [], eas.LENGTH, 0)], got[2]
    assert [(m.syncs, m.eoms, m.complete, m.lost, m.truncated) for m in models] == [(1, 0, 0, 0, 1), (1, 0, 0, 1, 0), (1, 1, 0, 0, 1)]
    last = models[1].events[-1]
    assert sum(e.flags == eas.BAD for e in models[1].events) == 3 and (last.code, last.flags, last.index) == (eas.LOST, eas.END, 7)


@on_gpu
def test_bad_bytes_lost_length_and_wrong_sync_bits(gpu):
    """what a clean alert never does, on the device: a START with errs above 0, of a header and of an end of message; BAD
    events and the run they count; an end by `lose` and an end by max_len, with their counters.  Status and events equal the
    model's after every call, from host and from device memory, and the model took each of these paths"""
    x = _damaged()
    n = x.shape[1]
    for device in (False, True):
        bank = SameBank(FS, B, 3, 8192, **DAMAGED_BANK)
        for s in range(3):
            bank.set(s, same_params(source=s))
        models = _models(bank, 3)
        st = _run(x, bank, models, range(3), _chunks(n, (1, 4096, 611, 8192)), device=device)
        _damaged_paths(models)
        assert [int(st[s]["lost"]) for s in range(3)] == [0, 1, 0] and [int(st[s]["truncated"]) for s in range(3)] == [1, 0, 1]
        assert [int(st[s]["eoms"]) for s in range(3)] == [0, 0, 1]
        assert [e.errs for e in (bank.event(0, 0), bank.event(2, 0))] == [3, 2] and bank.event(2, 0).code == ord("N")
        bank.close()


@functools.lru_cache(maxsize=None)
def _alert():
    """the whole alert on two rows: three headers, the 1050 Hz attention signal (cut to half a second), three ends of
    message, a second between the bursts; noise at 20 dB.  ([2][n] float32, read-only)"""
    xs = [eas.modulate(TEXT, FS, attention="weather", attention_seconds=0.5, amp=0.3, lead=0.05 + s * 3.7 / FS, tail=0.05)
          for s in range(2)]
    n = max(len(x) for x in xs)
    out = np.zeros((2, n), np.float32)
    for s, x in enumerate(xs):
        out[s, :len(x)] = x
        out[s] += np.random.default_rng(700 + s).normal(0.0, sm.noise_sigma(0.3, 20.0, FS), n).astype(np.float32)
    out.setflags(write=False)
    return out


@on_gpu
def test_the_whole_alert_with_its_ends_of_message(gpu):
    """three headers, the attention signal, three NNNN: the end-of-message pattern, its START event and `eoms` on the
    device, and nothing filed for the attention signal"""
    x = _alert()
    n = x.shape[1]
    bank = _bank(2, 16384)
    models = _models(bank, 2)
    st = _run(x, bank, models, range(2), _chunks(n, (16384, 4097, 9000)))
    for s, m in enumerate(models):
        bursts = eas.read(m.events)
        assert [(b.kind, b.text, b.errs) for b in bursts] == [("Z", TEXT, 0)] * 3 + [("N", "NNNN", 0)] * 3, bursts
        assert (m.syncs, m.eoms, m.complete) == (3, 3, 3) and int(st[s]["eoms"]) == 3
        assert int(st[s]["sync_sample"]) == bursts[-1].start_sample and [a.text for a in eas.vote(bursts, FS)] == [TEXT]
    bank.close()


@on_gpu
def test_the_whole_stream_in_one_call_against_random_cuts(gpu):
    x = _rows()
    n = x.shape[1]
    assert 200000 < n < 250000
    bank = _bank(ROWS, n)
    st = bank.process(x)
    for s, (status, events) in enumerate(_whole()):
        assert _status(st[s]) == status, (s, _status(st[s]), status)
        assert tuple(bank.events(s)) == events, s
    bank.close()
    cuts = _random_cuts(n, 1)
    assert any(b - a == 1 for a, b in cuts) and any(a % B and b % B and b - a > B for a, b in cuts) and len(cuts) > 100
    bank = _bank(ROWS, 4096)
    models = _models(bank, ROWS)
    st = _run(x, bank, models, range(ROWS), cuts)
    for s, (status, events) in enumerate(_whole()):                  # the same end, however the stream was cut
        assert _status(st[s]) == status and tuple(models[s].events) == events
    bank.close()


def _lanes(ncall, Lmin=1):
    """kq_gridbank.hpp's lanes_for_call for this geometry (B = 8: 64 frames of stride 10 fit the tile, so Lmin = 1)"""
    nf = (ncall + B - 2) // B + 1
    L = Lmin
    while L < 64 and 2 * L * nf <= 64:
        L *= 2
    return L


@on_gpu
def test_every_number_of_lanes_to_a_frame(gpu):
    """calls of 1, 5, 20, 50, 100, 200 and 400 samples take 64, 32, 16, 8, 4, 2 and 1 lanes to a frame; they walk through the
    first burst's preamble, sync and text, between calls of 4096"""
    sizes = (1, 5, 20, 50, 100, 200, 400)
    assert [_lanes(m) for m in sizes] == [64, 32, 16, 8, 4, 2, 1]
    x = _rows()
    n = 60000                                                        # the first burst and what lies ahead of the second
    cuts = _chunks(n, sizes + (611, 4096))
    bank = _bank(ROWS, 4096)
    models = _models(bank, ROWS)
    _run(x, bank, models, range(ROWS), cuts)
    assert all(m.complete == 1 and eas.read(m.events)[0].text == TEXT for m in models)
    bank.close()


@on_gpu
@pytest.mark.parametrize("device,fmt", [(False, kq.KQ_PCM_S16BE), (True, kq.KQ_PCM_F32), (True, kq.KQ_PCM_S16BE)])
def test_int16_and_device_input(gpu, device, fmt):
    """KQ_PCM_S16BE words, the word -32768 among them, from host memory; float and int16 from device memory in padded rows
    with junk between them.  (Host float is every other case's input)"""
    x = _rows()
    n = x.shape[1]
    s16 = fmt == kq.KQ_PCM_S16BE
    data = x
    if s16:
        data = sm.fm.quantise(x, 32767.0).astype(np.int16)
        data[:, 5:2000:7] = -32768
        data[0, -3:] = -32768
    bank = _bank(ROWS, 8192)
    models = _models(bank, ROWS)
    _run(data, bank, models, range(ROWS), _chunks(n, (1000, 8192, 4097)), device=device, fmt=fmt, s16=s16)
    for m in models:
        _read_whole(m.events)
    bank.close()


@on_gpu
def test_slots_that_share_a_row_and_exchanged_tones(gpu):
    """slots 0..3 on their rows; slots 4 and 5 on row 0 again, 5 with mark and space exchanged: it hears every bit turned
    over, finds neither pattern and files nothing; slot 6 on row 2 at 700 baud, which is no SAME"""
    x = _rows()
    n = x.shape[1]
    src = (0, 1, 2, 3, 0, 0, 2)
    bank = SameBank(FS, B, len(src), 8192)
    for s, r in enumerate(src):
        bank.set(s, same_params(source=r))
    bank.set(5, same_params(source=0, mark=sm.SPACE, space=sm.MARK))
    bank.set(6, same_params(source=2, baud=700.0))
    models = _models(bank, len(src))
    assert models[5].incs == models[0].incs[::-1] and models[6].tb != models[2].tb
    st = _run(x, bank, models, src, _chunks(n, (4096, 8192, 3001)))
    assert bank.events(4) == bank.events(0) and _status(st[4]) == _status(st[0])
    _read_whole(models[4].events)
    assert not models[5].events and models[5].syncs == 0 and int(bank.counts()[5]) == 0 and int(st[5]["events"]) == 0
    assert models[5].frames == n // B and any(v for _, v in models[5].bits)      # its gate did open: the patterns kept it out
    assert models[6].syncs == 0
    bank.close()


@on_gpu
def test_a_slot_set_inside_a_burst_removed_and_the_bank_reset(gpu):
    """slot 2 is set in the middle of the first burst's text, inside a frame, and sees zeros before it: it misses that burst
    and reads the other two; a removed slot stops and keeps its arena; reset starts the grid over, every slot cold"""
    x = _rows()
    n = x.shape[1]
    first = int(0.5 * FS) + 3                                        # half a second in: the first burst's text
    src = {0: 0, 1: 1, 3: 3}
    bank = SameBank(FS, B, ROWS, n)
    for s in range(ROWS):
        bank.set(s, same_params(source=s))
    models = _models(bank, ROWS)
    bank.remove(2)
    assert first % B and models[0].feed(x[0, :first]).synced == 1
    models[0] = _model(bank, 0)
    for a, b in ((0, first), (first, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, _snap(models), st, slots=list(src), what=(a, b))
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, same_params(source=2))
            src[2] = 2
            models[2] = _model(bank, 2, start=first)
    assert (models[2].syncs, models[2].complete) == (2, 2) and int(st[2]["frames"]) == (n - first // B * B) // B
    assert [b.text for b in eas.read(models[2].events)] == [TEXT] * 2
    # a removed slot stops: nothing is written for it, its arena stays; the others go on
    bank.remove(0)
    kept = bank.events(0)
    del src[0]
    st = bank.process(x[:, :first])
    for s, r in src.items():
        models[s].feed(x[r, :first])
    assert not st[0].tobytes().strip(b"\0") and bank.events(0) == kept and len(kept) == len(models[0].events)
    _check(bank, _snap(models), st, slots=list(src))
    assert int(st[1]["synced"]) == 1                                # the reset below falls inside a burst
    # reset: the grid starts over and every slot still set restarts cold, its sync discarded
    bank.reset()
    fresh = list(models)
    for s in src:
        fresh[s] = _model(bank, s)
    st = bank.process(x)
    for s, r in src.items():
        fresh[s].feed(x[r])
    _check(bank, _snap(fresh), st, slots=list(src))
    assert _status(st[1]) == _whole()[1][0] and tuple(bank.events(1)) == _whole()[1][1]
    bank.close()


@on_gpu
def test_an_arena_of_eight_events_fills_and_clear_events_between_the_bursts(gpu):
    """max_events = 8: a burst files 40 events, of which the arena keeps eight and counts the rest in `dropped`;
    kq_same_clear_events between the bursts empties the arenas and leaves status, register and clock alone"""
    x = _rows()
    n = x.shape[1]
    per_burst = 1 + len(TEXT) - 4 + 1
    gaps = [int((0.05 + (k + 1) * 8 * (16 + len(TEXT)) / eas.BAUD + (k + 0.5) * 1.0) * FS) for k in range(2)]   # mid-pause
    bank = _bank(ROWS, n, max_events=8)
    models = _models(bank, ROWS)
    at = 0
    for k, cut in enumerate(gaps + [n]):
        st = _run(x, bank, models, range(ROWS), [(at, cut)])
        at = cut
        for s in range(ROWS):
            assert int(bank.counts()[s]) == 8 and int(st[s]["events"]) == (k + 1) * per_burst
            assert int(st[s]["dropped"]) == (k + 1) * (per_burst - 8) and int(st[s]["synced"]) == 0
        bank.clear_events()
        for m in models:
            m.clear_events()
        assert not bank.counts().any()
    assert all(m.syncs == 3 and m.complete == 3 for m in models)
    bank.close()


@on_gpu
def test_16384_slots_for_one_burst(gpu):
    """every slot of the largest bank over the four rows, slot s on row s % 4, for the first burst: 64 slots spread over the
    bank (the first and the last workgroup among them) are held against the model, events and all; every other slot's
    status and arena count against the first slot of its row"""
    S = 16384
    x = _rows()[:, :52000]
    bank = SameBank(FS, B, S, 4096, max_events=48)
    for s in range(S):
        bank.set(s, same_params(source=s % ROWS))
    row_models = _models(bank, ROWS)                                 # slots 0..3: the rows' first slots
    picked = sorted(set(range(0, 60 * (S // 60), S // 60)) | {S - 4, S - 3, S - 2, S - 1})
    assert len(picked) == 64 and {s % ROWS for s in picked} == set(range(ROWS))
    for a, b in _chunks(x.shape[1], (4096, 4095, 1)):
        st = bank.process(x[:, a:b])
        for r, m in enumerate(row_models):
            m.feed(x[r, a:b])
        want = [m.status() for m in row_models]
        for s in picked:
            assert _status(st[s]) == want[s % ROWS], (a, b, s)
        for r in range(ROWS):
            mates = st[r::ROWS]
            for name in STATUS_DTYPE.names:
                assert (mates[name] == mates[name][0]).all(), (a, b, r, name)
    counts = bank.counts()
    for r, m in enumerate(row_models):
        assert m.complete == 1 and eas.read(m.events)[0].text == TEXT and (counts[r::ROWS] == len(m.events)).all()
    for s in picked:
        assert bank.events(s) == row_models[s % ROWS].events, s
    bank.close()


@on_gpu
@pytest.mark.parametrize("Fs,Bg", [(48000.0, 11), (39062.5, 8), (39062.5, 9), (96000.0, 23)])
def test_the_other_geometries(gpu, Fs, Bg):
    """the longest frame at 48 kHz, both frames of a receiver bank's 39 062.5 Hz, and the longest at 96 kHz: one burst on two rows, from host and from device memory"""
    x = _rows(Fs, 1, 2)
    n = x.shape[1]
    for device in (False, True):
        bank = SameBank(Fs, Bg, 2, 8192)
        for s in range(2):
            bank.set(s, same_params(source=s))
        models = _models(bank, 2)
        _run(x, bank, models, range(2), _chunks(n, (1, Bg - 1, Bg, Bg + 1, 80, 4096, 8192)), device=device)
        assert all(m.complete == 1 and eas.read(m.events)[0].text == TEXT for m in models)
        bank.close()


# ---- loopback: an AFSK-keyed USB station through a receiver bank's LINEAR channel, decoded in place ----
RF, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256          # 48 kHz audio into the modulator and out of the receiver


@on_gpu
def test_loopback_through_the_receiver(gpu):
    """SAME audio from eas.modulate into a USB station; a receiver bank with a LINEAR channel of 1300 to 2400 Hz at 48 kHz.
    The decode in place on the bank's stream (SameBank.beside, process_bank) must read the finished plane: status and events
    equal what the model makes of the same plane pulled to the host, and the header is the one sent."""
    per_call = 64
    rate = RF // INTERP
    La = LB // INTERP
    Bl = eas.same_config(rate)["block_len"]
    assert rate == 48000 and Bl == 9
    lead_in = eas.afsk(np.ones(300, np.uint8), rate, amp=0.5)[1]    # a steady tone that lets the receiver's gain settle
    audio = np.concatenate([lead_in, eas.modulate(TEXT, rate, eom=False, repeats=1, amp=0.5, lead=0.02, tail=0.05)])
    calls = -(-len(audio) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([audio, np.zeros(n - len(audio))]).astype(np.float32)[None, :]
    mod = kq.ModBank(RF, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(RF, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("usb", frequency=f, amplitude_dbfs=-20.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_LINEAR_DEMOD, low=1300.0, high=2400.0, second_lo=-f))
    same = SameBank.beside(rx, Bl, 1)
    assert same.samprate == rate and same.max_samples == per_call * La
    same.set(0, same_params(0))
    model = _model(same, 0)
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)        # receiver noise
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(same.process_bank(rx))                                  # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    got = same.events(0)
    bursts = eas.read(got)
    print("same loopback:", bursts, _status(st[0]))
    assert got == model.events
    assert [(b.kind, b.text, b.reason) for b in bursts] == [("Z", TEXT, eas.COMPLETE)]
    for h in (mod, rx, same):
        h.close()
