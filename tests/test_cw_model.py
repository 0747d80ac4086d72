"""What the CW decoder of include/ka9q_hip.h (kq_cw_*), as tests/cw_model.py restates it, decodes: seeded, no GPU.  The GPU
tests hold the kernel equal to this model with no tolerance, so what is shown here holds for the bank.

Noise is stated as the tone's power over the noise power in Fs / B, one frame's bandwidth: sigma^2 = (0.3^2 / 2) /
10^(dB / 10) * B / 2 (cw_model.noise_sigma)."""
import functools

import numpy as np
import pytest

import cw_model as cm
from ka9q_sdr_amd import morse

TEXT = "CQ CQ DE K1ABC K1ABC PSE K 5NN TU 73 QRZ W9XYZ"
AMP, LEAD, PITCH = 0.3, 0.5, 700.0
GRID = [(12000.0, 48), (39062.5, 128)]


@functools.lru_cache(maxsize=None)
def _clean(Fs, wpm):
    x = morse.encode(TEXT, wpm, Fs, PITCH, AMP, lead=LEAD)
    x.setflags(write=False)
    return x


def _decode(Fs, B, wpm, start, db, seed, **kw):
    x = _clean(Fs, wpm)
    if db is not None:
        x = x + np.random.default_rng(seed).normal(0.0, cm.noise_sigma(AMP, db, B), len(x)).astype(np.float32)
    m = cm.CwModel(Fs, B, pitch=PITCH, wpm=start, **kw).feed(x)
    return morse.read_text(m.events), m


def _distance(a, b):
    """Levenshtein"""
    d = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        p, d[0] = d[0], i
        for j, cb in enumerate(b, 1):
            p, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, p + (ca != cb))
    return d[-1]


def test_alphabet_and_encoder():
    assert morse.ALPHABET["A"] == 0b101 and morse.ALPHABET["E"] == 0b10 and morse.ALPHABET["0"] == 0b111111
    assert morse.ALPHABET["<SK>"] == morse.code_of("...-.-") and morse.elements_of(morse.ALPHABET["<AR>"]) == ".-.-."
    assert morse.elements_of(morse.ALPHABET["?"]) == "..--.." and len(morse.CHARACTERS) == len(morse.ALPHABET) >= 26 + 10 + 4 + 10
    assert all(2 <= c < 512 for c in morse.CHARACTERS)               # a leading 1 and at most 8 elements
    assert sum(d for _, d in morse.keying("PARIS E")[:-2]) == 50     # the standard word, with its gap
    assert morse.keying("E E") == [(True, 1), (False, 7), (True, 1), (False, 3)]
    x = morse.encode("E", 20, 12000.0, 700.0, 0.3, rise_ms=5.0, lead=0.1, tail=0.1)
    assert x.dtype == np.float32 and len(x) == round((0.1 + 4 * 0.06 + 0.1) * 12000)
    env = np.abs(x)
    assert env[:1100].max() == 0 and 0.29 < env[1300:1800].max() <= 0.3 and env[2100:].max() == 0
    assert 0.05 < np.abs(x[1195:1206]).max() < 0.25                  # half way up the leading edge
    Ev = cm.Event
    ev = [Ev(0b101, 2, 0, 0, 0, 0), Ev(1, 0, 0, 0, 0, 0), Ev(0, 9, 0, 0, 0, 0), Ev(morse.ALPHABET["<BT>"], 5, 0, 0, 0, 0),
          Ev(0b1010101010, 9, 0, 0, 0, 0), Ev(1, 0, 0, 0, 0, 0)]
    assert morse.read_text(ev) == "A ?<BT>?"
    assert morse.cw_config(12000.0, 75.0)["block_len"] == 48 and morse.cw_config(12000.0, 60.0)["block_len"] == 60
    assert morse.cw_config(39062.5, 60.0)["block_len"] == 195
    for fs, w in ((12000.0, 75.0), (12000.0, 60.0), (8000.0, 40.0), (48000.0, 60.0), (39062.5, 60.0)):
        c = morse.cw_config(fs, w)
        assert cm.unit_limits(fs, c["block_len"], c["min_wpm"], c["max_wpm"])[0] >= 64          # four frames in a dot


@pytest.mark.parametrize("db,cap", [(40.0, 0.0), (20.0, 0.05)])
def test_decodes_the_grid(db, cap):
    """(12000, 48) and (39062.5, 128), 12, 20 and 30 WPM from a start of 20, five seeds each: whole in every run at 40 dB;
    at 20 dB a character error rate of at most 5 % over the 30 runs (measured: 29 runs whole, one -- 30 WPM at 39062.5 Hz,
    where a dash of 586 sixteenths meets 2 u = 586 at the start -- with 24 of its 46 characters lost: 1.7 %)"""
    errs = whole = 0
    for Fs, B in GRID:
        for wpm in (12, 20, 30):
            for seed in range(5):
                got, m = _decode(Fs, B, wpm, 20.0, db, seed)
                errs += _distance(got, TEXT)
                whole += got == TEXT
                assert m.dropped == 0
    print("CW grid at %g dB: %d of 30 whole, CER %.4f" % (db, whole, errs / (30.0 * len(TEXT))))
    assert errs <= cap * 30 * len(TEXT)
    if db == 40.0:
        assert whole == 30


def test_acquires_from_a_start_speed_that_is_off():
    """16, 25 and 40 WPM from start speeds 0.7 and 1.4 times that, at (12000, 48) and 20 dB, five seeds each: whole"""
    bad = []
    for wpm in (16, 25, 40):
        for f in (0.7, 1.4):
            for seed in range(5):
                got, m = _decode(12000.0, 48, wpm, wpm * f, 20.0, seed)
                if got != TEXT:
                    bad.append((wpm, f, seed, got))
                assert abs(m.u - cm.unit_start(12000.0, 48, wpm)) <= cm.unit_start(12000.0, 48, wpm) // 4
    assert not bad, bad


def test_start_speed_off_by_two_locks_within_the_text():
    """40 WPM from a start of 20: at u = 240 a dash of 360 is below 2 u and reads as a dot, so u hovers between dots and
    dashes until a run of dots pulls it below 180.  The text's longest such run is the 5 of 5NN; the words behind it must
    read.  Characters lost ahead of that are printed, not asserted (measured: the first 6 words, 23 characters, read as
    ??H???E; from K on the text is whole)."""
    got, m = _decode(12000.0, 48, 40, 20.0, 20.0, 0)
    tail = "TU 73 QRZ W9XYZ"
    kept = 0
    while kept < len(TEXT) and got.endswith(TEXT[len(TEXT) - kept - 1:]):
        kept += 1
    print("CW 40 WPM from 20: read %r, lost the first %d characters" % (got, len(TEXT) - kept))
    assert got.endswith(tail), got
    assert abs(m.u - 120) <= 30


def test_noise_alone_gives_no_characters():
    x = np.random.default_rng(1).normal(0.0, 0.1, 60 * 12000).astype(np.float32)
    m = cm.CwModel(12000.0, 48).feed(x)
    assert m.frames == 15000 and [e for e in m.events if e.code != 1] == []
    assert m.hi < 16 * m.lo                                          # the peak stays within 12 dB of the floor


def test_steady_carrier_gives_no_characters_and_the_floor_follows():
    n = np.arange(10 * 12000)
    x = (AMP * np.sin(2 * np.pi * PITCH / 12000.0 * n)).astype(np.float32)
    m = cm.CwModel(12000.0, 48).feed(x)
    assert [e for e in m.events if e.code > 1] == []
    assert m.lo > m.P[-1] * 7 // 8 and m.key == 0
    # a carrier that comes up behind silence keys once, reads as one undecodable mark, and the floor takes it in
    x = np.concatenate([np.zeros(12000, np.float32), x])
    m = cm.CwModel(12000.0, 48).feed(x + np.random.default_rng(2).normal(0, 1e-3, len(x)).astype(np.float32))
    assert [e.code for e in m.events if e.code != 1] in ([], [0])
    assert m.lo > m.P[-1] * 3 // 4 and m.key == 0


def _keyed(Fs, pattern, dot=0.06, lead=0.5):
    """marks and spaces in dots, hard keyed"""
    out = [np.zeros(int(lead * Fs))]
    for mark, dots in pattern:
        out.append(np.full(int(round(dots * dot * Fs)), 1.0 if mark else 0.0))
    env = np.concatenate(out)
    return (AMP * env * np.sin(2 * np.pi * PITCH / Fs * np.arange(len(env)))).astype(np.float32)


def test_a_mark_of_nine_dots_is_undecodable():
    """a dot, then a mark of 9 dots: the character is undecodable.  (Beyond 8 dots the floor follows the mark, so the key
    comes up before the mark ends: its measured end lies between 8 and 9 dots behind its start.)"""
    x = _keyed(12000.0, [(True, 1), (False, 1), (True, 9), (False, 12)])
    m = cm.CwModel(12000.0, 48, wpm=20.0).feed(x)
    chars = [e for e in m.events if e.code != 1]
    assert [(e.code, e.nelem) for e in chars] == [(0, 2)]
    assert morse.read_text(m.events) == "?"
    assert chars[0].start_sample == 6000 and 10 * 720 < chars[0].end_sample - 6000 <= 11 * 720 + 48


def test_a_ninth_element_is_undecodable():
    eight = [(True, 1), (False, 1)] * 7 + [(True, 3), (False, 12)]
    nine = [(True, 1), (False, 1)] * 8 + [(True, 3), (False, 12)]
    m = cm.CwModel(12000.0, 48, wpm=20.0).feed(_keyed(12000.0, eight + nine))
    assert [(e.code, e.nelem) for e in m.events if e.code != 1] == [(0b100000001, 8), (0, 9)]
    assert [e.code for e in m.events] == [0b100000001, 1, 0, 1]


def test_call_splits_change_nothing():
    """the same stream in calls of 1, 47, 48, 49, 80 and 4096 samples, and in one piece: events and status identical"""
    x = _clean(12000.0, 30)[:70000]
    x = x + np.random.default_rng(3).normal(0.0, cm.noise_sigma(AMP, 20.0, 48), len(x)).astype(np.float32)
    whole = cm.CwModel(12000.0, 48, wpm=20.0).feed(x)
    assert len(whole.events) >= 10 and whole.I != 0                   # the stream ends inside a frame
    for sizes in ((1, 47, 48, 49, 80, 4096), (4096,), (80,), (49,)):
        m, at, k = cm.CwModel(12000.0, 48, wpm=20.0), 0, 0
        while at < len(x):
            n = sizes[k % len(sizes)]
            m.feed(x[at:at + n])
            at += n
            k += 1
        assert m.events == whole.events and m.status() == whole.status(), sizes
    assert whole.widest < 2 ** 55
