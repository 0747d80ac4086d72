"""What the PSK decoder of include/ka9q_hip.h (kq_psk_*), as tests/psk_model.py restates it, decodes: seeded, no GPU.  The
GPU tests hold the kernel equal to this model with no tolerance, so what is shown here holds for the bank.

The traffic is shaped BPSK from varicode.modulate at amplitude 0.3 behind 64 reversals.  Noise is white and stated as
Es/N0, the symbol's energy taken at the carrier's level: sigma^2 = (0.3^2 / 2) / 10^(dB / 10) * Fs / (2 baud)
(psk_model.noise_sigma)."""
import difflib
import functools
import math

import numpy as np
import pytest

import psk_model as pm
from ka9q_sdr_amd import varicode

AMP, LEAD, PITCH = 0.3, 64, 1000.0
GRID = [(12000.0, 24, 31.25), (8000.0, 16, 31.25), (39062.5, 50, 31.25), (12000.0, 12, 62.5), (12000.0, 8, 125.0),
        (48000.0, 96, 31.25)]
OFFSETS = (0.0, 1.0, -3.0, 5.0)
PPM = 100.0
TEXT = "CQ CQ de K1ABC K1ABC pse k. The quick brown fox jumps over the lazy dog 0123456789"
SEEDS = 5


def _random_text(seed, n=171):
    return "".join(chr(c) for c in np.random.default_rng(500 + seed).integers(32, 127, n))


@functools.lru_cache(maxsize=None)
def _traffic(seed):
    text = _random_text(seed)
    x = varicode.modulate(text, 12000.0, 31.25, PITCH, AMP, lead=LEAD)
    x.setflags(write=False)
    return text, x


def _noisy(x, db, Fs, baud, seed):
    return x + np.random.default_rng(seed).normal(0.0, pm.noise_sigma(AMP, db, Fs, baud), len(x)).astype(np.float32)


def _lost(got, sent):
    """characters of `sent` that `got` does not match in order"""
    sm = difflib.SequenceMatcher(None, list(got), list(sent), autojunk=False)
    return len(sent) - sum(b.size for b in sm.get_matching_blocks())


@pytest.mark.parametrize("Fs,B,baud", GRID)
def test_clean_copy_is_whole_on_the_grid(Fs, B, baud):
    """the signal 0, +1, -3 and +5 Hz off the slot's pitch from a sender whose clock is 100 ppm fast: the text whole, and the
    offset the events report of the right sign and within 0.5 Hz from the hundredth symbol on.  (The sender's carrier is
    100 ppm fast too: 0.1 Hz at 1 kHz.)"""
    for off in OFFSETS:
        x = varicode.modulate(TEXT, Fs, baud, PITCH + off, AMP, lead=LEAD, ppm=PPM)
        m = pm.PskModel(Fs, B, PITCH, baud).feed(x)
        assert varicode.read_text(m.events) == TEXT and m.dropped == 0 and not any(e.flags for e in m.events), (Fs, B, baud, off)
        true = (PITCH + off) * (1.0 + PPM * 1e-6) - PITCH
        late = [e for e in m.events if e.end_sample >= (LEAD + 100) / baud * Fs]
        assert len(late) > 20
        for e in late:
            got = varicode.offset_hz(e, baud)
            assert abs(got - true) < 0.5 and (off == 0.0 or got * off > 0), (Fs, B, baud, off, got, true)


def test_symbol_lengths_of_the_grid():
    assert [pm.symbol_length(Fs, B, baud) for Fs, B, baud in GRID] == [4096, 4096, 6400, 4096, 3072, 4096]
    assert [pm.window(pm.symbol_length(Fs, B, baud)) for Fs, B, baud in GRID] == [16, 16, 25, 16, 12, 16]
    assert pm.window(2048) == 8 and pm.window(8192) == 32
    for Fs, B, baud in GRID:
        assert varicode.psk_config(Fs, baud) == dict(block_len=B if B != 50 else 78)
    with pytest.raises(ValueError):
        varicode.psk_config(8000.0, 250.0)                               # four samples to a frame of sixteen: below B = 8


@pytest.mark.parametrize("db", [20.0, 14.0, 12.0, 10.0, 8.0], ids=lambda d: "%gdB" % d)
def test_copy_under_noise(db):
    """(12000, 24, 31.25), snr = 32, five seeds of 171 random printable characters each.  Whole at an Es/N0 of 20 dB.  Below
    that the loss is printed, not asserted (measured: none at 14 dB, 0.7 % at 12 dB, 19 % at 10 dB, 77 % at 8 dB)"""
    Fs, B, baud = 12000.0, 24, 31.25
    lost = 0
    for seed in range(SEEDS):
        text, x = _traffic(seed)
        m = pm.PskModel(Fs, B, PITCH, baud).feed(_noisy(x, db, Fs, baud, seed))
        got = varicode.read_text(m.events)
        if db >= 20.0:
            assert got == text and m.dropped == 0, seed
        lost += _lost(got, text)
    print("PSK31 (12000, 24) at %g dB: %d of %d characters lost (%.1f %%)" % (db, lost, SEEDS * 171, 100.0 * lost / (SEEDS * 171)))


def test_noise_alone_files_nothing():
    """120 s of Gaussian noise at (12000, 24), 31.25 baud, with the default snr of 32"""
    x = np.random.default_rng(0).normal(0.0, 0.1, 120 * 12000).astype(np.float32)
    m = pm.PskModel(12000.0, 24, PITCH, 31.25).feed(x)
    assert m.frames == 60000 and m.events == [] and m.nevents == 0
    assert m.sig >= m.min_p and len(m.bits) > 3700                    # the level is there: the ratio is what refuses it


def test_a_steady_carrier_files_nothing():
    n = np.arange(20 * 12000)
    for f, sigma in ((PITCH, 0.0), (PITCH + 2.0, 0.02)):
        x = (AMP * np.cos(2 * np.pi * f / 12000.0 * n)).astype(np.float32)
        x = x + np.random.default_rng(1).normal(0.0, sigma, len(n)).astype(np.float32) if sigma else x
        m = pm.PskModel(12000.0, 24, PITCH, 31.25).feed(x)
        assert m.events == [] and m.nevents == 0
        assert sum(v for _, v in m.bits) > 600 and all(b for b, v in m.bits if v)      # read, and all ones: no gap ever


def test_start_phase_and_polarity_change_nothing():
    """the code is differential"""
    Fs, B, baud = 12000.0, 24, 31.25
    for kw in (dict(phase=math.pi), dict(invert=True), dict(phase=1.0)):
        x = varicode.modulate(TEXT, Fs, baud, PITCH, AMP, lead=LEAD, **kw)
        m = pm.PskModel(Fs, B, PITCH, baud).feed(x)
        assert varicode.read_text(m.events) == TEXT, kw
    a = varicode.modulate(TEXT, Fs, baud, PITCH, AMP, lead=LEAD)
    assert np.allclose(varicode.modulate(TEXT, Fs, baud, PITCH, AMP, lead=LEAD, invert=True), -a, atol=1e-6)


def test_call_splits_change_nothing():
    """the same stream in calls of 1, B - 1, B, B + 1, 80 and 4096 samples, and in one piece: events and status identical"""
    Fs, B, baud = 12000.0, 24, 31.25
    _, x = _traffic(1)
    x = _noisy(x, 14.0, Fs, baud, 3)[:90001]
    whole = pm.PskModel(Fs, B, PITCH, baud).feed(x)
    assert len(whole.events) >= 10 and any(whole.acc)                 # the stream ends inside a frame
    for sizes in ((1, B - 1, B, B + 1, 80, 4096), (4096,), (80,), (B + 1,), (B - 1,)):
        m, at, k = pm.PskModel(Fs, B, PITCH, baud), 0, 0
        while at < len(x):
            n = sizes[k % len(sizes)]
            m.feed(x[at:at + n])
            at += n
            k += 1
        assert m.events == whole.events and m.status() == whole.status(), sizes
    m = pm.PskModel(Fs, B, PITCH, baud)
    for v in x[:3000]:
        m.feed(np.array([v]))
    assert m.status() == pm.PskModel(Fs, B, PITCH, baud).feed(x[:3000]).status()


def test_a_character_longer_than_ten_bits_is_flagged():
    Fs, B, baud = 12000.0, 24, 31.25
    e_, sp = [1, 1, 0, 0], [1, 0, 0]
    long11, long16 = [1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1], [1] * 16
    bits = e_ + long11 + [0, 0] + e_ + long16 + [0, 0] + sp + e_
    m = pm.PskModel(Fs, B, PITCH, baud).feed(varicode.modulate(bits, Fs, baud, PITCH, AMP, lead=LEAD))
    got = [(e.code, e.flags) for e in m.events]
    assert got == [(3, 0), (0b10111101111, 1), (3, 0), (0xFFF, 1), (1, 0), (3, 0)], got   # 16 ones: the last 12 and the flag
    assert varicode.read_text(m.events) == "e_e_ e".replace("_", varicode.REPLACEMENT)
    # ten ones: no character of the table, not flagged, and still a replacement character
    m = pm.PskModel(Fs, B, PITCH, baud).feed(varicode.modulate(e_ + [1] * 10 + [0, 0] + e_, Fs, baud, PITCH, AMP, lead=LEAD))
    assert [(e.code, e.flags) for e in m.events] == [(3, 0), (1023, 0), (3, 0)]
    assert varicode.read_text(m.events) == "e_e".replace("_", varicode.REPLACEMENT)


def test_a_full_arena_counts_what_it_drops():
    Fs, B, baud = 12000.0, 24, 31.25
    x = varicode.modulate("eeeeeeeeee", Fs, baud, PITCH, AMP, lead=LEAD)
    m = pm.PskModel(Fs, B, PITCH, baud, max_events=4).feed(x)
    assert len(m.events) == 4 and m.nevents == 10 and m.dropped == 6
    m.clear_events()
    m.feed(varicode.modulate("ee", Fs, baud, PITCH, AMP, lead=4))
    assert len(m.events) >= 1 and m.nevents == 10 + len(m.events)


def test_widest_intermediates_stay_inside_the_header_bounds():
    """a clipping square wave on the pitch, reversed now and then, through the longest window of the longest frames, and a
    noisy run at (12000, 24)"""
    Fs, B = 48000.0, 256
    baud = Fs / (B * 32.0)                                           # tb = 8192, W = 32
    n = np.arange(400 * B)
    x = np.sign(np.cos(2 * np.pi * 1000.0 / Fs * n)).astype(np.float32) * 4.0
    x[150 * B:250 * B] *= -1.0
    m = pm.PskModel(Fs, B, 1000.0, baud, snr=4095).feed(x)
    assert m.tb == 8192 and m.W == 32
    seen = dict(m.widest)
    _, gx = _traffic(0)
    g = pm.PskModel(12000.0, 24, PITCH, 31.25).feed(_noisy(gx, 10.0, 12000.0, 31.25, 0))
    seen = {k: max(v, g.widest[k]) for k, v in seen.items()}
    print("PSK widest:", {k: "2^%.1f" % math.log2(max(v, 1)) for k, v in seen.items()})
    assert seen["acc"] < 2 ** 38 and seen["red"] < 2 ** 25 and seen["sum"] < 2 ** 30
    assert seen["P"] < 2 ** 61 and seen["D"] < 2 ** 61 and seen["R"] < 2 ** 61 and seen["lvl"] < 2 ** 61
    assert seen["n"] <= 2 ** 24 and seen["dec"] <= 2 ** 49 and seen["prod"] < 2 ** 61
    assert seen["sum"] > 2 ** 28 and seen["D"] > 2 ** 57              # the case does reach up there


def test_the_table_has_its_structure_and_round_trips():
    V = varicode.VARICODE
    assert len(V) == 128 and len(set(V)) == 128
    assert all("00" not in s and s[0] == "1" and s[-1] == "1" and set(s) <= {"0", "1"} for s in V)
    short = [s for s in V if len(s) <= 9]
    every = {s for s in (bin(v)[2:] for v in range(1, 1 << 9)) if "00" not in s and s[-1] == "1"}
    assert len(every) == 88 and set(short) == every
    assert sum(len(s) == 10 for s in V) == 40 and max(len(s) for s in V) == 10
    assert V[ord("e")] == "11" and V[ord(" ")] == "1" and V[ord("t")] == "101" and V[ord("E")] == "1110111"
    assert varicode.CODES[ord("e")] == 3 and varicode.encode("e ") == [1, 1, 0, 0, 1, 0, 0]
    Ev = pm.Event
    text = "".join(chr(c) for c in range(128))
    bits = varicode.encode(text)
    codes = [int(s, 2) for s in "".join(map(str, bits)).split("00") if s]
    assert varicode.read_text([Ev(c, 0, 0, 0, 1, 0) for c in codes]) == text
    odd = [Ev(3, 0, 0, 0, 1, 0), Ev(3, 1, 0, 0, 1, 0), Ev(0b1001, 0, 0, 0, 1, 0)]              # e, e flagged, no character's code
    assert varicode.read_text(odd) == "e" + 2 * varicode.REPLACEMENT
    with pytest.raises(ValueError):
        varicode.encode("\u00e9")
    x = varicode.modulate("e", 12000.0, 31.25, PITCH, 0.3, lead=8, tail=4)
    assert x.dtype == np.float32 and len(x) == 16 * 384 and 0.29 < np.abs(x).max() <= 0.3
    assert abs(varicode.offset_hz(Ev(0, 0, 0, 0, 1000, -1000), 31.25) - 31.25 / 8) < 1e-9   # clockwise: above the pitch
