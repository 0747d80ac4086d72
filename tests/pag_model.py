"""Plain-loop restatement of the POCSAG pager decoder bank's algorithm (include/ka9q_hip.h, kq_pag_*) on the front end of
tests/fsk_model.py (quantiser, low-pass, threshold and bit clock are FskModel's, untouched), and a generator of test
traffic whose encoder is written apart from ka9q_sdr_amd.pocsag.encode, so that the two check each other.  Everything
after the quantiser is integer arithmetic, so the bank must give the model's records bit for bit."""
import numpy as np

import fsk_model as fm

FSC, IDLE = 0x7CD215D8, 0x7A89C197
LOST, FULL, BAD = 1, 2, 4
G_BITS = [1, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1]          # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1, highest power first
M32 = 0xFFFFFFFF

# the geometries the tests run: Fs, bit/s, K, W (W follows from window_bits = min(24, 1024 baud / Fs - 0.5))
CASES = [(19200.0, 1200, 31, 384), (48000.0, 2400, 41, 480), (8192.0, 512, 31, 384), (48000.0, 1200, 63, 960),
         (39062.5, 2400, 31, 391), (22050.0, 1200, 31, 441)]


def default_window(Fs, baud):
    return min(24.0, 1024.0 * baud / Fs - 0.5)


# ---- the code, by long division on lists of bits ----
def _remainder(bits31):
    r = list(bits31)
    for i in range(21):
        if r[i]:
            for j, g in enumerate(G_BITS):
                r[i + j] ^= g
    return r[21:]


def make_word(data21):
    """21 data bits (flag, payload) -> the 32-bit codeword"""
    d = [data21 >> (20 - i) & 1 for i in range(21)]
    bits = d + _remainder(d + [0] * 10)
    bits.append(sum(bits) & 1)
    return int("".join(map(str, bits)), 2)


def syndrome(x):
    r = _remainder([x >> (31 - i) & 1 for i in range(31)])
    return int("".join(map(str, r)), 2)


def _patterns():
    t = {(0, 0): 0}
    for i in range(32):
        t[(syndrome(1 << i), 1)] = 1 << i
        for j in range(i):
            e = 1 << i | 1 << j
            t[(syndrome(e), 0)] = e
    assert len(t) == 1 + 32 + 496
    return t


PATTERNS = _patterns()


def correct(x):
    """(v, e), or (None, -1)"""
    e = PATTERNS.get((syndrome(x), bin(x).count("1") & 1))
    if e is None:
        return None, -1
    return x ^ e, bin(e).count("1")


class PagModel(fm.FskModel):
    """One slot.  feed() takes the next samples of the stream; pages, counters and the status fields are the bank's."""

    def __init__(self, Fs, baud, K, cutoff_hz=None, beta=2.0, window_bits=None, input_scale=4096.0, pll_shift=3, max_pages=16,
                 max_page_words=64, taps=None, start=0):
        super().__init__(Fs, baud, K, scrambled=False, cutoff_hz=0.75 * baud if cutoff_hz is None else cutoff_hz, beta=beta,
                         window_bits=default_window(Fs, baud) if window_bits is None else window_bits, input_scale=input_scale,
                         pll_shift=pll_shift, taps=taps, start=start)
        self.max_pages, self.mpw = max_pages, max_page_words
        self.sh = self.synced = self.inv = self.cnt = self.pos = self.miss = 0
        self.page = None                         # the open page: [ric, function, [3-byte words], flags, errors, end_sample]
        self.syncs = self.batches = self.sync_missed = 0
        self.words_good = self.words_fixed = self.words_bad = self.orphans = self.npages = self.dropped = 0
        self.pages = []                          # the arena: (ric, function, words, flags, errors, end_sample)

    def clear_pages(self):
        self.pages = []

    def _close(self, flag=0):
        p = self.page
        self.page = None
        self.npages += 1
        if len(self.pages) < self.max_pages:
            self.pages.append((p[0], p[1], b"".join(p[2]), p[3] | flag, p[4], p[5]))
        else:
            self.dropped += 1

    def _append(self, x, code):
        p = self.page
        p[2].append((code << 20 | x >> 11 & 0xFFFFF).to_bytes(3, "big"))
        p[5] = self.n

    def _channel_bit(self, c):
        self.bits += 1
        self.sh = (self.sh << 1 | c) & M32
        if not self.synced:
            for inv, w in ((0, self.sh), (1, self.sh ^ M32)):
                if bin(w ^ FSC).count("1") <= 2:
                    self.synced, self.inv = 1, inv
                    self.cnt = self.pos = self.miss = 0
                    self.syncs += 1
                    self.batches += 1
                    break
            return
        self.cnt += 1
        if self.cnt < 32:
            return
        self.cnt = 0
        x = self.sh ^ M32 if self.inv else self.sh
        if self.pos == 16:
            self.pos = 0
            if bin(x ^ FSC).count("1") <= 2:
                self.batches += 1
                self.miss = 0
                return
            self.sync_missed += 1
            self.miss += 1
            if self.miss == 2:
                self.synced = 0
                if self.page:
                    self._close(LOST)
            return
        before = self.pos
        self.pos += 1
        v, e = correct(x)
        if e < 0:
            self.words_bad += 1
            if self.page and len(self.page[2]) < self.mpw:
                self._append(x, 3)
                self.page[3] |= BAD
            return
        if e:
            self.words_fixed += 1
        else:
            self.words_good += 1
        if v == IDLE:
            if self.page:
                self._close()
        elif not v >> 31:
            if self.page:
                self._close()
            self.page = [(v >> 13 & 0x3FFFF) << 3 | before >> 1, v >> 11 & 3, [], 0, e, self.n]
        elif not self.page:
            self.orphans += 1
        elif len(self.page[2]) < self.mpw:
            self._append(v, e)
            self.page[4] += e
        else:
            self._close(FULL)
            self.orphans += 1

    def status(self):
        return dict(bits=self.bits, syncs=self.syncs, batches=self.batches, sync_missed=self.sync_missed,
                    words_good=self.words_good, words_fixed=self.words_fixed, words_bad=self.words_bad, orphans=self.orphans,
                    pages=self.npages, dropped=self.dropped, pll_phase=self.s, synced=self.synced, inverted=self.inv,
                    level=self.level)


# ---- generator ----
def train(pages):
    """pages = [(ric, function, payloads)] -> every codeword of the transmission, the FSCs among them: batches of FSC + 16
    places, an address in places 2 (ric & 7) of a batch, its message behind it, IDLE elsewhere and at least once at the end"""
    places = {}                                  # place number (16 a batch) -> codeword
    at = 0
    for ric, function, payloads in pages:
        want = 2 * (ric & 7)
        at += (want - at) % 16
        places[at] = make_word((ric >> 3) << 2 | function)
        for k, p in enumerate(payloads):
            places[at + 1 + k] = make_word(1 << 20 | p)
        at += 1 + len(payloads)
    nbatch = at // 16 + 1
    out = []
    for b in range(nbatch):
        out.append(FSC)
        out += [places.get(16 * b + k, IDLE) for k in range(16)]
    return out


def word_bits(words):
    return [w >> (31 - i) & 1 for w in words for i in range(32)]


def preamble():
    return [1, 0] * 288


def longest_run(bits):
    b = np.asarray(bits)
    edges = np.flatnonzero(np.diff(b)) + 1
    return int(np.diff(np.concatenate([[0], edges, [len(b)]])).max())


def flip(words, every=3, first=1, seed=0, nflips=2):
    """nflips distinct bits flipped in words first, first + every, ...; returns (words, the indices touched)"""
    rng = np.random.default_rng(seed)
    out, hit = list(words), []
    for i in range(first, len(out), every):
        for b in rng.choice(32, nflips, replace=False):
            out[i] ^= 1 << int(b)
        hit.append(i)
    return out, hit


def make_pages(count, seed, lo=1, hi=6):
    """random pages: (ric, function, payloads)"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(8, 1 << 21)), int(rng.integers(0, 4)), [int(v) for v in rng.integers(0, 1 << 20, int(rng.integers(lo, hi)))])
            for _ in range(count)]


def pag_signal(bits, Fs, baud, ppm=0.0, amp=0.3, dc=0.05, noise=0.0, seed=0, invert=False, lead=0.01, tail=0.02):
    """the line bits as a two-level signal (a 1 is the upper level, or the lower one with invert), shaped as fsk_model.shape
    does, between `lead` and `tail` seconds of silence; plus dc and white noise all along.  float32, rad/sample"""
    sig = amp * fm.shape(bits, Fs, baud, ppm)
    if invert:
        sig = -sig
    x = np.concatenate([np.zeros(int(lead * Fs)), sig, np.zeros(int(tail * Fs))]) + dc
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(len(x))
    return x.astype(np.float32)


def sent(pages):
    """what a decoder makes of pages that arrive whole: (ric, function, payloads, flags)"""
    return [(ric, function, list(payloads), 0) for ric, function, payloads in pages]


def got(pages):
    """the arena's records in the form of sent(): the error codes and end_sample left out"""
    out = []
    for ric, function, words, flags, errors, end in pages:
        vals = [int.from_bytes(words[k:k + 3], "big") for k in range(0, len(words), 3)]
        out.append((ric, function, [v & 0xFFFFF for v in vals], flags))
    return out
