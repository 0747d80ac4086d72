"""The POCSAG pager decoder's algorithm on the CPU (tests/pag_model.py, the restatement the GPU tests compare with): it gives
back exactly the pages that were sent at six geometries (pag_model.CASES: 8 192 to 48 000 Hz, 512 to 2400 bit/s, 16 to 40
samples per bit), over clock error, noise and either polarity, with two flipped bits in every third codeword; its encoder
and ka9q_sdr_amd.pocsag.encode, written apart, make the same bits; the alphabets round-trip; and the deframer's seams (a sync word with two errors, missed sync words, full
and damaged pages, orphans) at the level of channel bits."""
import numpy as np
import pytest

import pag_model as pm
from ka9q_sdr_amd import pocsag

AMP, DC = 0.3, 0.05


def _bits_of(pages, corrupt=True, seed=0):
    words = pm.train(pages)
    hit = []
    if corrupt:
        words, hit = pm.flip(words, seed=seed)
    return words, hit, pm.preamble() + pm.word_bits(words)


@pytest.mark.parametrize("Fs,baud,K,W", pm.CASES)
def test_model_recovers_every_page(Fs, baud, K, W):
    """cutoff 0.75 baud, pll_shift 3, window_bits min(24, 1024 baud / Fs - 0.5): every codeword sent comes back, every
    batch is found, and the records say which words were mended"""
    seed = 500 + 20 * pm.CASES.index((Fs, baud, K, W))
    for ppm in (0.0, 100.0, -100.0):
        for noise in (0.0, 0.03, 0.06):
            for invert in (False, True):
                pages = pm.make_pages(5, seed)
                clean = pm.train(pages)
                words, hit, bits = _bits_of(pages, seed=seed)
                assert pm.longest_run(bits) <= 21
                x = pm.pag_signal(bits, Fs, baud, ppm, AMP, DC, noise, seed, invert, lead=16.0 / baud, tail=20.0 / baud)
                m = pm.PagModel(Fs, baud, K)
                assert m.W == W
                m.feed(x)
                st = m.status()
                what = (ppm, noise, invert, st)
                assert pm.got(m.pages) == pm.sent(pages), what
                nb = len(words) // 17
                assert (st["syncs"], st["batches"], st["sync_missed"], st["inverted"]) == (1, nb, 0, int(invert)), what
                mended = [i for i in hit if i % 17]
                assert (st["words_good"], st["words_fixed"], st["words_bad"]) == (16 * nb - len(mended), len(mended), 0), what
                assert (st["orphans"], st["pages"], st["dropped"]) == (0, len(pages), 0), what
                assert sum(p[4] for p in m.pages) == 2 * sum(clean[i] != pm.IDLE for i in mended), what
                ends = [p[5] for p in m.pages]
                assert ends == sorted(ends) and ends[-1] < len(x)
                seed += 1


PAGE_SETS = [
    [(8, 0, [])],                                                     # tone only, frame 0
    [(15, 3, [0xFFFFF, 0])],                                          # frame 7: the message runs into the next batch
    [(1234567, 1, list(range(40)))],                                  # over three batches
    [(9, 0, [1] * 13)],                                               # ends with the batch: a batch of IDLE follows
    [(10, 0, [5]), (10, 1, []), (11, 2, [7, 8]), (9, 3, [9])],        # same frame twice; a frame that has gone by
    pm.make_pages(12, 3),
]


@pytest.mark.parametrize("pages", PAGE_SETS)
def test_the_two_encoders_make_the_same_bits(pages):
    words, bits = pocsag.encode(pages, 1200)
    mine = pm.train(pages)
    assert words.dtype == np.uint32 and bits.dtype == np.uint8
    assert words.tolist() == mine and bits.tolist() == pm.preamble() + pm.word_bits(mine)
    assert len(mine) % 17 == 0 and all(w == pm.FSC for w in mine[::17]) and mine[-1] == pm.IDLE
    for (ric, function, payloads) in pages:
        at = mine.index(pocsag.address_word(ric, function))
        assert (at % 17 - 1) // 2 == ric & 7
    for w in mine:
        assert pm.correct(w) == (w, 0)
    with pytest.raises(ValueError):
        pocsag.encode(pages, 9600)


def test_constants_and_codewords():
    assert (pocsag.FSC, pocsag.IDLE, pocsag.GENERATOR) == (0x7CD215D8, 0x7A89C197, 0x769)
    assert (pocsag.LOST, pocsag.FULL, pocsag.BAD) == (pm.LOST, pm.FULL, pm.BAD) == (1, 2, 4)
    assert pocsag.codeword(pm.FSC >> 11) == pm.FSC and pocsag.codeword(pm.IDLE >> 11) == pm.IDLE
    assert pm.make_word(pm.FSC >> 11) == pm.FSC and pm.make_word(pm.IDLE >> 11) == pm.IDLE
    rng = np.random.default_rng(2)
    for d in rng.integers(0, 1 << 21, 200):
        assert pocsag.codeword(int(d)) == pm.make_word(int(d))


def _run_bits(bits, **kw):
    """the deframer alone: channel bits in, one per `sample`"""
    m = pm.PagModel(19200.0, 1200, 31, **kw)
    for b in bits:
        m._channel_bit(int(b))
        m.n += 1
    return m


def _page(m, k):
    return pocsag.Page(*m.pages[k])


def test_alphabets_round_trip():
    for text in ("0123456789", "*U -][", "555 1212", "7", "12345", "1 2 3 4 5 6"):
        m = _run_bits(pocsag.encode([(77, 0, pocsag.numeric_payloads(text))])[1])
        assert pocsag.numeric(_page(m, 0)) == text and pocsag.numeric(m.pages[0][2]) == text
    for text in ("A", "AB", "ABC", "Hello, world", "20 chars exactly here", "x" * 97, "tab\tand~{}"):
        m = _run_bits(pocsag.encode([(1000, 3, pocsag.alpha_payloads(text))])[1])
        assert pocsag.alpha(_page(m, 0)) == text, text
        assert m.pages[0][:2] == (1000, 3)
    # EOT and ETX fill is stripped as NUL is
    bits = [c >> i & 1 for c in (ord("H"), ord("i"), 4, 3, 0) for i in range(7)] + [0] * 5
    raw = b"".join(int("".join(map(str, bits[k:k + 20])), 2).to_bytes(3, "big") for k in (0, 20))
    assert pocsag.alpha(raw) == "Hi"
    with pytest.raises(ValueError):
        pocsag.alpha_payloads("é")


def test_uncorrectable_word_reads_as_question_marks():
    pages = [(77, 3, pocsag.alpha_payloads("ABCDEFGHIJK"))]           # 77 bits: four words
    words = pm.train(pages)
    at = words.index(pocsag.address_word(77, 3)) + 2                  # the second message word: bits 20..39
    words[at] ^= 0b111 << 12
    m = _run_bits(pm.preamble() + pm.word_bits(words))
    p = _page(m, 0)
    assert p.flags == pm.BAD and p.errors == 0 and len(p.words) == 12 and p.words[3] >> 4 == 3
    assert m.status()["words_bad"] == 1
    assert pocsag.alpha(p) == "AB????GHIJK"                           # characters 2..5 have bits in 20..39
    pages = [(77, 0, pocsag.numeric_payloads("1234567890"))]
    words = pm.train(pages)
    words[words.index(pocsag.address_word(77, 0)) + 1] ^= 0b10101 << 3
    m = _run_bits(pm.preamble() + pm.word_bits(words))
    assert pocsag.numeric(_page(m, 0)) == "?????67890"


def test_sync_word_with_two_errors_is_accepted_three_are_not():
    pages = pm.make_pages(3, 9, lo=6, hi=9)
    clean = pm.train(pages)
    assert len(clean) == 3 * 17
    for where in (0, 17):
        words = list(clean)
        words[where] ^= 1 << 30 | 1 << 2
        m = _run_bits(pm.preamble() + pm.word_bits(words))
        st = m.status()
        assert pm.got(m.pages) == pm.sent(pages) and (st["syncs"], st["batches"], st["sync_missed"]) == (1, 3, 0), where
    # either polarity
    m = _run_bits([1 - b for b in pm.preamble() + pm.word_bits(clean)])
    assert pm.got(m.pages) == pm.sent(pages) and m.status()["inverted"] == 1
    # three errors in the first sync word: the first batch is not seen at all
    words = list(clean)
    words[0] ^= 0b111 << 9
    m = _run_bits(pm.preamble() + pm.word_bits(words))
    st = m.status()
    assert (st["syncs"], st["batches"]) == (1, 2) and st["words_good"] == 32


def test_one_missed_sync_word_is_ridden_through_two_close_the_page_with_lost():
    pages = [(8, 2, list(range(100, 160)))]                           # 61 words from place 0: into the fourth batch
    clean = pm.train(pages)
    assert len(clean) == 4 * 17
    words = list(clean)
    words[17] ^= 0xFF00                                               # the second batch's sync word: missed
    m = _run_bits(pm.preamble() + pm.word_bits(words))
    st = m.status()
    assert pm.got(m.pages) == pm.sent(pages)
    assert (st["syncs"], st["batches"], st["sync_missed"], st["synced"]) == (1, 3, 1, 1)
    words[34] ^= 0xFF00                                               # and the third: sync is dropped there
    m = _run_bits(pm.preamble() + pm.word_bits(words))
    st = m.status()
    assert pm.got(m.pages) == [(8, 2, list(range(100, 131)), pm.LOST)]    # the address and 31 words of two batches
    assert (st["syncs"], st["batches"], st["sync_missed"]) == (2, 2, 2)   # found again at the fourth batch's sync word
    assert st["orphans"] == 60 - 31 - 16 and st["pages"] == 1
    assert m.pages[0][5] == 576 + 34 * 32 - 1                         # the last stored codeword ends ahead of that sync word


def test_full_pages_orphans_and_the_arena():
    pages = [(8, 0, [1, 2, 3, 4, 5]), (9, 1, []), (10, 2, [6])]
    words = pm.train(pages)
    bits = pm.preamble() + pm.word_bits(words)
    m = _run_bits(bits, max_page_words=3)
    st = m.status()
    # the fourth word finds the page full and closes it; it and the fifth are orphans
    assert pm.got(m.pages) == [(8, 0, [1, 2, 3], pm.FULL), (9, 1, [], 0), (10, 2, [6], 0)]
    assert (st["orphans"], st["pages"], st["dropped"]) == (2, 3, 0)
    m = _run_bits(bits, max_pages=2)
    assert pm.got(m.pages) == pm.sent(pages)[:2] and (m.status()["pages"], m.status()["dropped"]) == (3, 1)
    # a message word with no address in front of it
    lone = [pm.FSC] + [pm.IDLE, pm.make_word(1 << 20 | 99)] + [pm.IDLE] * 14
    m = _run_bits(pm.preamble() + pm.word_bits(lone))
    assert m.pages == [] and m.status()["orphans"] == 1 and m.status()["words_good"] == 16


def test_model_is_invariant_to_splitting():
    Fs, baud, K, _ = pm.CASES[4]
    pages = pm.make_pages(4, 31)
    _, _, bits = _bits_of(pages, seed=31)
    x = pm.pag_signal(bits, Fs, baud, 100.0, AMP, DC, 0.03, 5, True)
    whole = pm.PagModel(Fs, baud, K)
    whole.feed(x)
    assert pm.got(whole.pages) == pm.sent(pages)
    rng = np.random.default_rng(8)
    for step in (1, 63, 64, 65, 1000, None):
        m = pm.PagModel(Fs, baud, K)
        at = 0
        while at < len(x):
            n = int(rng.integers(1, 300)) if step is None else step
            m.feed(x[at:at + n])
            at += n
        assert m.pages == whole.pages and m.status() == whole.status(), step
