"""The POCSAG pager decoder bank (kq_pag_*, ka9q_sdr_amd/csrc/kq_pag.hip) on the GPU against the integer model of
tests/pag_model.py: page records (ric, function, words with their error codes, flags, errors, end_sample), arena counts
and every status field equal, bit for bit, with no tolerance anywhere -- from host and device memory, float and
big-endian int16 input, padded rows, under other call splits, on 70 slots (two waves of the tracker), with pages carried
over calls and batches, tone-only, full, damaged and orphaned, a full arena, slots set mid-stream, removed, reset and
sharing a row, and in a loopback from a ModBank station through a receiver bank's flat FM channel.  The model runs on the
bank's own taps (kq_pag_get_taps; tests/test_pag_args.py holds them within one LSB of the model's design), so nothing in
the comparison is floating point but the quantiser's one multiply.  Where the input is one that tests/test_pag_model.py
has shown the model to decode completely (amplitude 0.3, DC 0.05, noise up to 0.06, +-100 ppm, either polarity), the pages
must also be those sent."""
import functools

import numpy as np
import pytest
import torch

import bank_gpu
import ka9q_sdr_amd as kq
import pag_model as pm
from ka9q_sdr_amd import pocsag
from ka9q_sdr_amd.pag import STATUS_DTYPE, STATUS_WORDS, TILE, PagBank, pag_params, status_array

pytestmark = pytest.mark.gpu


def _signal(words, Fs, baud, **kw):
    x = pm.pag_signal(pm.preamble() + pm.word_bits(words), Fs, baud, lead=16.0 / baud, tail=20.0 / baud, **kw)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _row(Fs, baud, s):
    """slot s's transmission: five pages in four to six batches, two flipped bits in every third codeword; clock error
    0 / +-100 ppm; amplitude 0.3, 0.05 or 1 rad/sample; DC 0.05 at amplitude 0.3, else up to half the amplitude; noise up
    to a tenth of the amplitude; the polarity by the slot's parity"""
    rng = np.random.default_rng(100 + s)
    pages = pm.make_pages(5, 300 + s % 7, lo=4, hi=8)
    words, _ = pm.flip(pm.train(pages), seed=s)
    assert 4 <= len(words) // 17 <= 6
    amp = (0.3, 0.05, 1.0)[s % 3]
    dc = 0.05 if s % 3 == 0 else amp * rng.uniform(-0.5, 0.5)
    return pages, _signal(words, Fs, baud, ppm=(0.0, 100.0, -100.0)[(s // 3) % 3], amp=amp, dc=dc,
                          noise=amp * (0.0, 0.03, 0.1)[(s // 2) % 3], seed=s, invert=s % 2 == 1)


def _stack(rows):
    """rows of one length: the shorter ones begin later, behind more of their idle level.  (Not in front of it: a steady
    level behind a transmission reads as zeros to a decoder still in sync, and the word 0 is a codeword, an address.)"""
    n = max(len(x) for x in rows)
    return np.array([np.concatenate([np.full(n - len(x), x[0], np.float32), x]) for x in rows])


def _rows(Fs, baud, S):
    rows = [_row(Fs, baud, s) for s in range(S)]
    return [p for p, _ in rows], _stack([x for _, x in rows])


def _shown(s):
    """slots whose level, DC and noise the CPU test covers: those must give back what was sent"""
    return s % 3 == 0


def _models(bank, S, **kw):
    hq = bank.get_taps()
    return [pm.PagModel(bank.samprate, bank.baud, bank.taps, taps=hq, window_bits=bank.window_bits, max_pages=bank.max_pages,
                        max_page_words=bank.max_page_words, **kw) for _ in range(S)]


def _setup(bank, S):
    for s in range(S):
        bank.set(s, pag_params(source=s))


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap, _chunks = functools.partial(bank_gpu.snap, "pages"), bank_gpu.chunks
_check = functools.partial(bank_gpu.check, _status, "page")
_device_call = functools.partial(bank_gpu.device_call, status_array)


# Fs, bit/s, K, slots: 16, 20 and 16 samples per bit; 70 slots put k_pag_track on two waves
PARITY = [(19200.0, 1200, 31, 70), (48000.0, 2400, 41, 3), (8192.0, 512, 31, 3)]


@pytest.mark.parametrize("Fs,baud,K,S", PARITY)
def test_parity_from_host_and_device_memory(gpu, Fs, baud, K, S):
    pages, x = _rows(Fs, baud, S)
    n = x.shape[1]
    assert n > 40 * TILE
    cap = n // 3 + 64
    cuts = _chunks(n, (cap, 257, n // 4))                    # several calls, none on a word boundary but the first
    want = None
    for device in (False, True):
        bank = PagBank(Fs, baud, K, S, cap)
        assert bank.get_taps().sum() in range(32768 - K, 32768 + K)
        _setup(bank, S)
        if want is None:                                     # the models' records after every call, made once
            models, want = _models(bank, S), []
            for a, b in cuts:
                for s, m in enumerate(models):
                    m.feed(x[s, a:b])
                want.append(_snap(models))
        st_t = torch.zeros((S, STATUS_WORDS), dtype=torch.int32, device="cuda")
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            if device:
                st = _device_call(bank, x[:, a:b], nblocks, st_t)
            else:
                st = bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, what=(device, a, b))
        bank.close()
    decoded = [pm.got(m.pages) == pm.sent(pages[s]) for s, m in enumerate(models)]
    print("pag parity %s: %d of %d slots decode every page" % ((Fs, baud, K, S), sum(decoded), S))
    assert all(decoded[s] for s in range(S) if _shown(s))
    assert all(m.status()["batches"] >= 4 for s, m in enumerate(models) if _shown(s))


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal far beyond the quantiser's range"""
    Fs, baud, K, S = 19200.0, 1200, 31, 2
    pages = [pm.make_pages(3, 40 + s) for s in range(S)]
    x = _stack([_signal(pm.train(p), Fs, baud, amp=20.0, dc=1.0, invert=bool(s)) for s, p in enumerate(pages)])
    assert (np.abs(x) * 4096 > 40000).mean() > 0.3          # 20 rad/sample x 4096: clips at +-32767
    words = pm.fm.quantise(x * np.float32(0.02), 4096.0).astype(np.int16)
    words[:, 5:40:7] = -32768
    words[0, -3:] = -32768
    st_t = torch.zeros((S, STATUS_WORDS), dtype=torch.int32, device="cuda")
    for data, fmt in ((x, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = PagBank(Fs, baud, K, S, 8192)
        _setup(bank, S)
        models = _models(bank, S)
        for a, b in _chunks(x.shape[1], (1000, 8192)):
            st = _device_call(bank, data[:, a:b], 1, st_t, fmt) if device else bank.process(data[:, a:b], 1, fmt)
            for s, m in enumerate(models):
                m.feed(data[s, a:b], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, a, b))
        assert all(pm.got(m.pages) == pm.sent(pages[s]) for s, m in enumerate(models))
        bank.close()


def test_call_splits_change_nothing(gpu):
    """the same stream in one call, and cut by 1, 63, 64, 65, 1000, 1024, 1025 and 7777 samples in turn, in one block or
    many: identical records (end_sample included), counts and status, those of the model fed in one piece"""
    Fs, baud, K, S = 19200.0, 1200, 31, 3
    pages, x = _rows(Fs, baud, S)
    n = x.shape[1]
    ref = None
    for sizes in ((n,), (1, 63, 64, 65, 1000, TILE, TILE + 1, 7777), (TILE - 1, 2 * TILE + 64, 7, 129)):
        bank = PagBank(Fs, baud, K, S, n)
        _setup(bank, S)
        if ref is None:
            models = _models(bank, S)
            for s, m in enumerate(models):
                m.feed(x[s])
            ref = _snap(models)
            assert [len(p) for _, p in ref] == [5, 5, 5] and pm.got(ref[0][1]) == pm.sent(pages[0])
        for a, b in _chunks(n, sizes):
            m = b - a
            nblocks = next(k for k in (8, 3, 2, 1) if m % k == 0)
            st = bank.process(x[:, a:b], nblocks)
        _check(bank, ref, st, what=sizes)
        bank.close()


def test_page_seams(gpu):
    """Row 0: a page whose message runs over a batch boundary, with a call boundary inside it.  Row 1: a tone-only page.
    Row 2: a message longer than max_page_words.  Row 3: a word with three flipped bits inside a page.  Row 4: a message
    word with no address.  Row 5: four pages into an arena of three, which clear_pages frees."""
    Fs, baud, K, S = 19200.0, 1200, 31, 6
    sets = [[(15, 1, list(range(1, 9)))],                    # frame 7: the address in place 14, seven words in the next batch
            [(8, 2, [])],
            [(9, 0, list(range(20, 32)))],
            [(10, 3, [0x12345, 0x6789A, 0xBCDEF])],
            [],
            [(8 + k, k, [k + 1]) for k in range(4)]]
    trains = [pm.train(p) for p in sets]
    at = trains[3].index(pocsag.address_word(10, 3)) + 2
    trains[3][at] ^= 0b1011 << 20
    trains[4][5] = pocsag.message_word(0x54321)
    x = _stack([_signal(w, Fs, baud, invert=k % 2 == 1) for k, w in enumerate(trains)])
    n = x.shape[1]
    spb = Fs / baud
    lead0 = n - len(_signal(trains[0], Fs, baud))            # row 0 begins here
    cut = lead0 + int((16 + 576 + 32 * 18 + 10) * spb)       # inside the first word of row 0's second batch
    bank = PagBank(Fs, baud, K, S, n, max_pages=3, max_page_words=8)
    _setup(bank, S)
    models = _models(bank, S)
    for a, b in ((0, cut), (cut, n)):
        st = bank.process(x[:, a:b])
        for s, m in enumerate(models):
            m.feed(x[s, a:b])
        _check(bank, _snap(models), st, what=(a, b))
        if a == 0:                                           # the page is open across the calls: not in the arena yet
            assert int(bank.counts()[0]) == 0 and int(st[0]["batches"]) == 2 and int(st[0]["words_good"]) == 16
    got = [pm.got(bank.pages(s)) for s in range(S)]
    assert got[0] == pm.sent(sets[0]) and got[1] == [(8, 2, [], 0)]
    assert got[2] == [(9, 0, list(range(20, 28)), pm.FULL)] and int(st[2]["orphans"]) == 4
    assert got[3] == [(10, 3, [0x12345, 0x6789A ^ 0b1011 << 9 & 0xFFFFF, 0xBCDEF], pm.BAD)] and int(st[3]["words_bad"]) == 1
    assert bank.pages(3)[0].words[3] >> 4 == 3 and pocsag.alpha(bank.pages(3)[0])[2:6] == "????"
    assert got[4] == [] and int(st[4]["orphans"]) == 1
    assert got[5] == pm.sent(sets[5])[:3] and (int(st[5]["pages"]), int(st[5]["dropped"])) == (4, 1)
    ends = [p.end_sample for p in bank.pages(5)]
    assert ends == sorted(ends) and 0 < ends[0] and ends[-1] < n
    # clear_pages empties the arenas and nothing else: the same stream again fills them again, the counters go on
    bank.clear_pages()
    assert not bank.counts().any()
    for m in models:
        m.clear_pages()
    st = bank.process(x)
    for s, m in enumerate(models):
        m.feed(x[s])
    _check(bank, _snap(models), st, what="again")
    # (a decoder still in sync from the first pass takes the preamble for codewords, which the alternating word is: message
    # words on an inverted row such as this one, orphans; addresses on the others, whose arenas the model fills alike)
    assert (int(st[5]["pages"]), int(st[5]["dropped"])) == (8, 2) and int(bank.counts()[5]) == 3
    assert pm.got(bank.pages(5)) == pm.sent(sets[5])[:3]
    assert bank.pages(5)[0].end_sample > n                   # end_sample runs on
    bank.close()


def test_slot_lifecycle(gpu):
    """Slots 0 and 3 share source row 0; slot 2 is set after the first call and sees zeros before it; a removed slot
    stops and keeps its arena; reset starts the grid over"""
    Fs, baud, K = 19200.0, 1200, 31
    rows = [_row(Fs, baud, s) for s in (0, 3)]              # both at the level the CPU test covers; row 1 inverted, +100 ppm
    pages, x = [p for p, _ in rows], _stack([v for _, v in rows])
    n = x.shape[1]
    first = 50                                               # inside a word, before any transmission begins
    bank = PagBank(Fs, baud, K, 4, n)
    src = {0: 0, 1: 1, 3: 0}
    for s, r in src.items():
        bank.set(s, pag_params(source=r))
    models = _models(bank, 4)
    late = _models(bank, 1, start=first)[0]
    for a, b in ((0, first), (first, n)):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        if a == 0:
            assert not st[2].tobytes().strip(b"\0")
            bank.set(2, source=1)
            src[2] = 1
        else:
            late.feed(x[1, a:b])
    models[2] = late
    _check(bank, _snap(models), st)
    assert bank.pages(0) == bank.pages(3) and pm.got(bank.pages(0)) == pm.sent(pages[0])
    assert pm.got(bank.pages(2)) == pm.got(bank.pages(1)) == pm.sent(pages[1])   # nothing was sent in the first 50 samples
    assert _status(st[2])["bits"] < _status(st[1])["bits"]
    # a removed slot stops: nothing is written for it, its arena stays; the others go on
    bank.remove(0)
    kept = bank.pages(0)
    st = bank.process(x)
    for s in (1, 2, 3):
        models[s].feed(x[src[s]])
    assert not st[0].tobytes().strip(b"\0") and bank.pages(0) == kept
    _check(bank, _snap(models), st, slots=[1, 2, 3])
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    fresh = _models(bank, 4)
    st = bank.process(x)
    for s in (1, 2, 3):
        fresh[s].feed(x[src[s]])
    _check(bank, _snap(fresh), st, slots=[1, 2, 3])
    assert bank.pages(1)[0].end_sample < n and bank.pages(0) == kept
    bank.close()


# ---- loopback: an FM station through a receiver bank, decoded in place ----
FS, INTERP, LB, MB, DRX = 12288000, 256, 8192, 8193, 256     # 48 kHz audio into the modulator and out of the receiver


def test_loopback_through_the_receiver(gpu):
    """A 2400 bit/s transmission keyed with pocsag.encode's bits on an FM station of 3 kHz deviation whose audio band
    passes DC to 7 kHz; a receiver bank with a flat FM channel at 48 kHz (20 samples per bit).  The decode in place on the
    bank's stream must read the finished plane: bit for bit what the model makes of the same plane pulled to the host,
    and every page sent comes out, in order, with its text."""
    per_call, baud, K = 64, 2400, 41
    rate = FS // INTERP
    La = LB // INTERP
    texts = ["ka9q-radio on gfx950", "0123 456-789"]
    sent_pages = [(1234567, 3, pocsag.alpha_payloads(texts[0])), (2001, 0, pocsag.numeric_payloads(texts[1])), (77, 1, [])]
    _, bits = pocsag.encode(sent_pages, baud)
    sig = pm.pag_signal(bits.tolist(), rate, baud, amp=1.0, dc=0.0, lead=0.0, tail=0.0)
    # The carrier stays up for 700 samples (35 bits, less the delay of the two filters) behind the last bit and the stream
    # ends there: a decoder stays in sync for two batches, and of the words that receiver noise makes one in four is within
    # two bits of a codeword, so a longer silence could add a page nobody sent.  The silence goes in front instead.
    tail = 700
    calls = -(-(len(sig) + 960 + tail) // (per_call * La))
    n = calls * per_call * La
    pcm = np.concatenate([np.zeros(n - len(sig) - tail, np.float32), sig, np.zeros(tail, np.float32)])[None, :]
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 1, per_call)
    assert rx.olen == La
    f = 1.0e6
    mod.set_station(0, kq.station_config("fm", frequency=f, amplitude_dbfs=-20.0, deviation=3000.0, low=-7000.0, high=7000.0))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-10000.0, high=10000.0, second_lo=-f, flat=1))
    pag = PagBank.beside(rx, baud, K, max_slots=1)
    assert pag.samprate == rate and pag.max_samples == per_call * La
    pag.set(0, source=0)
    model = _models(pag, 1)[0]
    rng = np.random.default_rng(11)
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        # Receiver noise, as in test_gpu_modulate, and more of it: this signal stays inside the channel filter, so its
        # envelope is steadier than float32 can tell from constant, and the squelch's amplitude variance (fm.c:91-103), a
        # small difference of large numbers, would come out <= 0 for some blocks and close it.  sigma 200 against a carrier
        # of 3277 is 49 dB in the 20 kHz channel: no bit is in doubt.
        noisy = s16.astype(np.float64) + rng.normal(0.0, 200.0, s16.shape)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        st = status_array(pag.process_bank(rx))                             # ordered after the decode
        model.feed(np.concatenate([rx.audio(0, b) for b in range(per_call)]))
        assert _status(st[0]) == model.status(), (c, _status(st[0]), model.status())
    print("pag loopback:", _status(st[0]))
    assert (int(st[0]["words_fixed"]), int(st[0]["words_bad"]), int(st[0]["batches"])) == (0, 0, 3)
    got = pag.pages(0)
    assert got == model.pages
    assert pm.got(got) == pm.sent(sent_pages), (pm.got(got), _status(st[0]))
    assert pocsag.alpha(got[0]) == texts[0] and pocsag.numeric(got[1]) == texts[1] and got[2].words == b""
    for h in (mod, rx, pag):
        h.close()
