"""What the RTTY decoder of include/ka9q_hip.h (kq_rtty_*), as tests/rtty_model.py restates it, decodes: seeded, no GPU.
The GPU tests hold the kernel equal to this model with no tolerance, so what is shown here holds for the bank.

The traffic is 60 random 5-bit characters sent back to back with 1.5 stop bits, continuous-phase FSK at amplitude 0.3
behind 2.5 s of mark.  Noise is white and stated as Eb/N0: sigma^2 = (0.3^2 / 2) / 10^(dB / 10) * Fs / (2 baud)
(rtty_model.noise_sigma)."""
import difflib
import functools
import math

import numpy as np
import pytest

import rtty_model as rm
from ka9q_sdr_amd import baudot

AMP, LEAD, MARK = 0.3, 2.5, 1500.0
GRID = [(12000.0, 24, 45.45, 170.0), (12000.0, 8, 50.0, 450.0), (39062.5, 64, 45.45, 170.0), (48000.0, 48, 100.0, 170.0)]
SEEDS = 5                # the runs asserted whole at 16 dB depend on these: other noise seeds lose a character in about one run
                         # of thirty at two of the geometries, so new seeds may need a look at the model, not at the test


@functools.lru_cache(maxsize=None)
def _traffic(Fs, baud, shift, seed, nbits=5):
    codes = np.random.default_rng(1000 + seed).integers(0, 1 << nbits, 60).tolist()
    x = baudot.encode(codes, baud, Fs, MARK, MARK + shift, AMP, nbits=nbits, lead=LEAD, tail=0.3)
    x.setflags(write=False)
    return tuple(codes), x


def _noisy(x, db, Fs, baud, seed):
    if db is None:
        return x
    return x + np.random.default_rng(seed).normal(0.0, rm.noise_sigma(AMP, db, Fs, baud), len(x)).astype(np.float32)


def _lost(got, sent):
    """characters of `sent` that `got` does not match in order"""
    sm = difflib.SequenceMatcher(None, list(got), list(sent), autojunk=False)
    return len(sent) - sum(b.size for b in sm.get_matching_blocks())


@pytest.mark.parametrize("db", [None, 20.0, 16.0, 14.0, 12.0], ids=lambda d: "clean" if d is None else "%gdB" % d)
def test_decodes_the_grid(db):
    """the four geometries, five seeds each: every run whole when clean, at 20 dB and at 16 dB.  At 14 dB and 12 dB the
    character error rate is printed, not asserted (measured over the 20 runs: 1.0 % at 14 dB, with 0 to 2.3 % per
    geometry; 9.7 % at 12 dB, with 7 to 14.3 %)"""
    lost = total = 0
    for Fs, B, baud, shift in GRID:
        here = 0
        for seed in range(SEEDS):
            codes, x = _traffic(Fs, baud, shift, seed)
            m = rm.RttyModel(Fs, B, MARK, MARK + shift, baud).feed(_noisy(x, db, Fs, baud, seed))
            got = [e.code for e in m.events]
            if db is None or db >= 16.0:
                assert got == list(codes) and m.ferr == 0 and m.dropped == 0, (Fs, B, baud, db, seed)
            here += _lost(got, codes)
        print("RTTY (%g, %d, %g baud, %g Hz) at %s: %d of %d characters lost" % (Fs, B, baud, shift, db, here, SEEDS * 60))
        lost += here
        total += SEEDS * 60
    print("RTTY grid at %s: character error rate %.4f" % (db, lost / total))


def test_bit_lengths_of_the_grid():
    assert [rm.bit_length(Fs, B, baud) for Fs, B, baud, _ in GRID] == [2816, 7680, 3438, 2560]
    assert [rm.window(rm.bit_length(Fs, B, baud)) for Fs, B, baud, _ in GRID] == [11, 30, 13, 10]
    assert rm.window(2048) == 8 and rm.window(8192) == 32


def test_noise_alone_gives_no_characters():
    """5 x 60 s of Gaussian noise at (12000, 24), 45.45 baud, with the default snr of 96"""
    for seed in range(5):
        x = np.random.default_rng(seed).normal(0.0, 0.1, 60 * 12000).astype(np.float32)
        m = rm.RttyModel(12000.0, 24, MARK, MARK + 170.0, 45.45).feed(x)
        assert m.frames == 30000 and m.events == [] and m.nevents == 0, seed
        assert m.sig >= m.min_p                                       # the level is there: the ratio is what refuses it


def test_steady_mark_gives_no_characters():
    n = np.arange(10 * 12000)
    x = (AMP * np.sin(2 * np.pi * MARK / 12000.0 * n)).astype(np.float32)
    m = rm.RttyModel(12000.0, 24, MARK, MARK + 170.0, 45.45).feed(x)
    assert m.events == [] and m.state == rm.IDLE and m.false_starts == 0 and all(m.levels[64:])
    assert m.sig > 100 * m.nse                                      # the window's response 170 Hz off is 24 dB down


def _keyed(Fs, baud, pattern, mark=MARK, space=MARK + 170.0):
    """marks and spaces in bits, continuous phase"""
    f = np.concatenate([np.full(int(round(bits / baud * Fs)), mark if m else space) for m, bits in pattern])
    return (AMP * np.sin(2.0 * np.pi * np.cumsum(f) / Fs)).astype(np.float32)


def test_a_false_start_counts_and_files_nothing():
    """a space of a third of a bit.  At a shift of 4.5 times the baud rate it turns the mark's phase by half a cycle
    (shift / (3 baud) = 1.5 cycles), so with the gap in the middle of the window the mark before it and the mark behind
    it cancel and the window reads space for a few frames; half a bit on, where the start bit is read, the window holds
    half the gap and mark behind it, and reads mark"""
    Fs, B, baud = 12000.0, 24, 50.0
    x = _keyed(Fs, baud, [(True, 100), (False, 1 / 3), (True, 30)], space=MARK + 225.0)
    m = rm.RttyModel(Fs, B, baud=baud, mark=MARK, space=MARK + 225.0).feed(x)
    assert 0 in m.levels[64:], "the dip must show for this test to mean anything"
    assert m.false_starts == 1 and m.events == [] and m.nevents == 0 and m.state == rm.IDLE
    # at 170 Hz and 45.45 baud the two marks are a quarter of a cycle apart and a third of a bit of space never outweighs
    # them: nothing starts at all
    x = _keyed(Fs, 45.45, [(True, 100), (False, 1 / 3), (True, 30)])
    m = rm.RttyModel(Fs, B, baud=45.45, mark=MARK, space=MARK + 170.0).feed(x)
    assert m.false_starts == 0 and m.events == [] and all(m.levels[64:])


def test_a_framing_error_is_flagged_and_the_slot_waits_for_mark():
    Fs, B, baud = 12000.0, 24, 45.45
    bits = lambda c: [(bool(c >> i & 1), 1) for i in range(5)]
    # a character whose stop element is space, and the space goes on (a break); then mark, and a good character
    pat = [(True, 100), (False, 1)] + bits(0b10101) + [(False, 6), (True, 10), (False, 1)] + bits(0b01110) + [(True, 10)]
    m = rm.RttyModel(Fs, B, baud=baud, mark=MARK, space=MARK + 170.0)
    x = _keyed(Fs, baud, pat)
    cut = int((100 + 1 + 5 + 3) / baud * Fs)                        # inside the break
    m.feed(x[:cut])
    assert [(e.code, e.flags) for e in m.events] == [(0b10101, 1)] and m.ferr == 1 and m.state == rm.WAIT
    m.feed(x[cut:])
    assert [(e.code, e.flags) for e in m.events] == [(0b10101, 1), (0b01110, 0)] and m.ferr == 1 and m.state == rm.IDLE
    assert baudot.read_text(m.events) == "C" and baudot.read_text(m.events, keep_framing_errors=True) == "YC"
    assert m.events[1].start_sample % B == 0 and m.events[0].sig > 16 * m.events[0].nse


@pytest.mark.parametrize("nbits", [7, 8])
def test_longer_characters_round_trip(nbits):
    Fs, B, baud = 12000.0, 24, 45.45
    codes, x = _traffic(Fs, baud, 170.0, 3, nbits)
    assert max(codes) >= 1 << (nbits - 1)
    m = rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud, nbits=nbits).feed(x)
    assert [e.code for e in m.events] == list(codes) and m.ferr == 0


def test_a_reversed_signal_reads_once_mark_and_space_are_swapped():
    Fs, B, baud = 12000.0, 24, 45.45
    codes, x = _traffic(Fs, baud, 170.0, 0)
    x = baudot.encode(list(codes), baud, Fs, MARK + 170.0, MARK, AMP, lead=LEAD, tail=0.3)      # sent upside down
    m = rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud).feed(x)
    assert [e.code for e in m.events if not e.flags] != list(codes)
    m = rm.RttyModel(Fs, B, MARK + 170.0, MARK, baud).feed(x)
    assert [e.code for e in m.events] == list(codes)


def test_call_splits_change_nothing():
    """the same stream in calls of 1, B - 1, B, B + 1, 80 and 4096 samples, and in one piece: events and status identical"""
    Fs, B, baud = 12000.0, 24, 45.45
    codes, x = _traffic(Fs, baud, 170.0, 1)
    x = _noisy(x, 16.0, Fs, baud, 3)[:60001]
    whole = rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud).feed(x)
    assert len(whole.events) >= 10 and any(whole.acc)                 # the stream ends inside a frame
    for sizes in ((1, B - 1, B, B + 1, 80, 4096), (4096,), (80,), (B + 1,), (B - 1,)):
        m, at, k = rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud), 0, 0
        while at < len(x):
            n = sizes[k % len(sizes)]
            m.feed(x[at:at + n])
            at += n
            k += 1
        assert m.events == whole.events and m.status() == whole.status(), sizes
    m = rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud)
    for v in x[:3000]:
        m.feed(np.array([v]))
    assert m.status() == rm.RttyModel(Fs, B, MARK, MARK + 170.0, baud).feed(x[:3000]).status()


def test_alphabet_round_trips_through_both_cases():
    assert baudot.LETTERS[1] == "E" and baudot.LETTERS[3] == "A" and baudot.LETTERS[4] == " " and baudot.LETTERS[16] == "T"
    assert baudot.LETTERS[25] == "B" and baudot.LETTERS[30] == "V" and baudot.LETTERS[8] == "\r" and baudot.LETTERS[2] == "\n"
    for ltr, fig in zip("QWERTYUIOP", "1234567890"):
        assert baudot.FIGURES[baudot.LETTERS.index(ltr)] == fig
    for ltr, fig in zip("ASDFGHJKLZXCVBNM", "-\a$!&#'()\"/:;?,."):
        assert baudot.FIGURES[baudot.LETTERS.index(ltr)] == fig, ltr
    assert baudot.codes_of("A1") == [31, 3, 27, 23] and baudot.codes_of("1 A") == [31, 27, 23, 4, 3]
    assert baudot.codes_of("1 2") == [31, 27, 23, 4, 27, 19]
    assert baudot.codes_of("1 2", unshift_on_space=False) == [31, 27, 23, 4, 19]
    Ev = rm.Event
    text = "RYRY CQ DE K1ABC 599 001 TU\r\nUR 5NN-73 $4.50 (OK)?"
    ev = [Ev(c, 0, 0, 0, 0) for c in baudot.codes_of(text)]
    assert baudot.read_text(ev) == text
    ev = [Ev(c, 0, 0, 0, 0) for c in baudot.codes_of(text, unshift_on_space=False)]
    assert baudot.read_text(ev, unshift_on_space=False) == text and baudot.read_text(ev) != text
    assert baudot.read_text([Ev(27, 0, 0, 0, 0), Ev(23, 0, 0, 0, 0), Ev(4, 0, 0, 0, 0), Ev(23, 0, 0, 0, 0)]) == "1 Q"
    assert baudot.read_text([Ev(0xE3, 0, 0, 0, 0), Ev(0, 0, 0, 0, 0), Ev(1, 1, 0, 0, 0)]) == "A"       # the low five bits
    with pytest.raises(ValueError):
        baudot.codes_of("a~b")
    assert baudot.rtty_config(12000.0, 45.45) == dict(block_len=26) and baudot.rtty_config(48000.0, 45.45)["block_len"] == 105
    assert baudot.rtty_config(3.0e6, 45.45)["block_len"] == 256
    for fs, baud in ((12000.0, 45.45), (12000.0, 50.0), (12000.0, 75.0), (39062.5, 45.45), (48000.0, 100.0), (8000.0, 75.0)):
        assert 2560 <= rm.bit_length(fs, baudot.rtty_config(fs, baud)["block_len"], baud) <= 8192
    with pytest.raises(ValueError):
        baudot.rtty_config(8000.0, 110.0)


def test_encoder_and_text_through_the_model():
    Fs, baud = 12000.0, 45.45
    x = baudot.encode("E", baud, Fs, 1000.0, 1170.0, 0.3, lead=0.1, tail=0.1)       # LTRS and E: two characters of 7.5 bits
    assert x.dtype == np.float32 and len(x) == round((0.2 + 15 / baud) * Fs) and 0.29 < np.abs(x).max() <= 0.3
    assert np.abs(np.diff(x)).max() < 0.3 * 2 * np.pi * 1170.0 / Fs * 1.01           # the phase is continuous
    text = "CQ DE K1ABC 599-001 (TU)"
    x = baudot.encode(text, baud, Fs, MARK, MARK + 170.0, AMP, lead=LEAD)
    m = rm.RttyModel(Fs, 24, MARK, MARK + 170.0, baud).feed(_noisy(x, 20.0, Fs, baud, 9))
    assert baudot.read_text(m.events) == text and [e.code for e in m.events] == baudot.codes_of(text)


def test_widest_intermediates_stay_inside_the_header_bounds():
    """a clipping square wave on the mark tone through the longest window of the longest frames, and a noisy run of each of
    the grid's geometries"""
    Fs, B = 48000.0, 256
    baud = Fs / (B * 32.0)                                           # tb = 8192, W = 32
    n = np.arange(200 * B)
    x = np.sign(np.sin(2 * np.pi * 1000.0 / Fs * n)).astype(np.float32) * 4.0
    m = rm.RttyModel(Fs, B, 1000.0, 1000.001, baud, snr=4095).feed(x)
    assert m.tb == 8192 and m.W == 32
    seen = dict(m.widest)
    for gFs, gB, gbaud, shift in GRID:
        _, gx = _traffic(gFs, gbaud, shift, 0)
        g = rm.RttyModel(gFs, gB, MARK, MARK + shift, gbaud).feed(_noisy(gx, 14.0, gFs, gbaud, 0))
        seen = {k: max(v, g.widest[k]) for k, v in seen.items()}
    print("RTTY widest:", {k: "2^%.1f" % math.log2(max(v, 1)) for k, v in seen.items()})
    assert seen["acc"] < 2 ** 38 and seen["red"] < 2 ** 26 and seen["sum"] < 2 ** 31
    assert seen["P"] < 2 ** 63 and seen["lvl"] < 2 ** 63 and seen["prod"] < 2 ** 75
    assert seen["sum"] > 2 ** 29                                      # the case does reach up there
