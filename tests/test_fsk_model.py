"""The FSK / GMSK packet decoder's algorithm on the CPU (tests/fsk_model.py, the restatement the GPU tests compare with): it
recovers what the generator sends over rates, slot kinds, clock error, DC, noise and level; scrambler and descrambler
are inverses; splitting the input changes nothing; the filter cannot overflow; and the AIS helpers on a known sentence."""
import numpy as np
import pytest

import fsk_model as fm
from common import ax25_fcs
from ka9q_sdr_amd.ais import ais_bits_from_nmea, ais_nmea, ais_payload_bits, ais_position

GRID = [(48000, 9600, 21), (39062, 9600, 17), (96000, 9600, 41), (48000, 4800, 41), (48000, 1200, 127)]
# amplitude, DC, noise sigma (rad/sample)
LEVELS = ((0.3, 0.15, 0.03), (0.3, -0.15, 0.03), (0.05, 0.0, 0.0), (2.5, 0.1, 0.0), (0.3, 0.0, 0.0))


def sent(frames):
    return [f + ax25_fcs(f) for f in frames]


def burst(Fs, baud, scrambled, seed, ppm=0.0, amp=0.3, dc=0.0, noise=0.0, count=3, **kw):
    """(frames, signal): a G3RUH burst behind 8 flags, or an AIS one behind the 24-bit preamble and two flags"""
    frames = fm.make_frames(count, seed)
    kw.setdefault("lead", 16.0 / baud)
    kw.setdefault("tail", 24.0 / baud)
    x = fm.fsk_signal(frames, Fs, baud, scrambled, ppm, amp, dc, noise, seed, preamble=not scrambled,
                      lead_flags=8 if scrambled else 2, **kw)
    return frames, x


@pytest.mark.parametrize("Fs,baud,K", GRID)
def test_model_recovers_every_frame(Fs, baud, K):
    """cutoff 0.6 baud, beta 2, window_bits 16 (the model's defaults).  The threshold needs both levels inside its window,
    so the seeds are ones whose scrambled stream has no run of window_bits equal bits"""
    run = 1000 + 30 * GRID.index((Fs, baud, K))
    for scrambled in (True, False):
        for ppm in (0.0, 100.0, -100.0):
            for amp, dc, noise in LEVELS:
                frames, x = burst(Fs, baud, scrambled, run, ppm, amp, dc, noise)
                m = fm.FskModel(Fs, baud, K, scrambled=scrambled)
                m.feed(x)
                assert [f[0] for f in m.frames] == sent(frames), (scrambled, ppm, amp, dc, noise, m.status())
                assert m.frames_good == 3 and m.dropped == 0
                ends = [f[1] for f in m.frames]
                assert ends == sorted(ends) and ends[-1] < len(x)
                run += 1


def test_scrambler_and_descrambler_are_inverses():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2, 2000).tolist()
    assert fm.descramble(fm.scramble(u)) == u
    # self-synchronising: a descrambler that starts anywhere in the stream is right after 17 bits
    c = fm.scramble(u)
    for at in (1, 13, 500):
        assert fm.descramble(c[at:])[17:] == u[at + 17:]
    # one channel-bit error comes out as three
    c[300] ^= 1
    bad = [i for i, (a, b) in enumerate(zip(fm.descramble(c), u)) if a != b]
    assert bad == [300, 312, 317]


def test_running_extrema_are_the_window_extrema():
    rng = np.random.default_rng(6)
    y = rng.integers(-2 ** 31, 2 ** 31, 700).astype(np.int64)
    for W in (2, 3, 4, 5, 7, 8, 63, 64, 65, 80, 699, 700):
        win = np.lib.stride_tricks.sliding_window_view(y, W)
        assert np.array_equal(fm.running(y, W, np.maximum), win.max(axis=1)), W
        assert np.array_equal(fm.running(y, W, np.minimum), win.min(axis=1)), W


@pytest.mark.parametrize("scrambled", [True, False])
def test_model_is_invariant_to_splitting(scrambled):
    frames, x = burst(39062, 9600, scrambled, 77, ppm=100.0, dc=0.1, noise=0.02, count=2)
    whole = fm.FskModel(39062, 9600, 17, scrambled=scrambled)
    whole.feed(x)
    assert [f[0] for f in whole.frames] == sent(frames)
    rng = np.random.default_rng(8)
    for step in (1, 63, 64, 65, 1000, None):
        m = fm.FskModel(39062, 9600, 17, scrambled=scrambled)
        at = 0
        while at < len(x):
            n = int(rng.integers(1, 300)) if step is None else step
            m.feed(x[at:at + n])
            at += n
        assert m.frames == whole.frames and m.status() == whole.status(), step


def test_filter_cannot_overflow():
    for Fs, baud, K in GRID + [(48000, 9600, 3), (48000, 9600, 127), (384000, 9600, 127)]:
        hq = fm.design_taps(K, 0.6 * baud, Fs, 2.0)
        assert np.abs(hq).sum() <= 65535 and abs(int(hq.sum()) - 32768) <= K
        assert np.abs(hq).sum() * 32767 < 2 ** 31
    # a long filter at four samples per bit has side lobes enough to break the bound: kq_fsk_create refuses it
    assert np.abs(fm.design_taps(127, 0.6 * 9600, 38400, 2.0)).sum() > 65535


def test_quantiser():
    x = np.array([0.0, 0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096, -1.5 / 4096, 7.9999, 8.0, -8.0, 100.0, -100.0, np.nan,
                  np.inf, -np.inf], np.float32)
    assert fm.quantise(x, 4096.0).tolist() == [0, 0, 2, 2, 0, -2, 32767, 32767, -32767, 32767, -32767, 0, 32767, -32767]
    assert fm.quantise(np.array([-32768, -32767, 32767, 5], np.int16), 4096.0, s16=True).tolist() == [-32767, -32767, 32767, 5]


def test_deframer_counts_bad_and_aborted_frames():
    """a flipped bit and a frame beyond max_frame_bytes land in frames_bad; seven ones inside a frame count in aborts"""
    Fs, baud, K = 48000, 9600, 21
    rng = np.random.default_rng(21)
    frames = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (20, 30, 20)]
    bits = fm.afsk_bits(frames)
    flip = list(bits)
    flip[8 * 8 + 41] ^= 1                                   # inside the first frame
    abort = bits[:8 * 8 + 60] + [1] * 9 + bits[8 * 8 + 60:]

    def run(stream, mfb=512):
        m = fm.FskModel(Fs, baud, K, scrambled=False, max_frame_bytes=mfb)
        sig = 0.3 * fm.shape(fm.line_bits(stream, False), Fs, baud)
        m.feed(np.concatenate([np.zeros(100), sig, np.zeros(200)]).astype(np.float32))
        return m

    m = run(bits)                                           # (the silence behind the burst reads as ones: one abort)
    assert (m.frames_good, m.frames_bad, m.aborts) == (3, 0, 1) and [f[0] for f in m.frames] == sent(frames)
    m = run(flip)
    assert (m.frames_good, m.frames_bad) == (2, 1) and [f[0] for f in m.frames] == sent(frames)[1:]
    m = run(bits, mfb=24)                                   # 22 and 32 bytes with the FCS
    assert (m.frames_good, m.frames_bad) == (2, 1) and [f[0] for f in m.frames] == [sent(frames)[0], sent(frames)[2]]
    m = run(abort)
    assert (m.frames_good, m.frames_bad, m.aborts) == (2, 0, 2) and [f[0] for f in m.frames] == sent(frames)[1:]


# ---- AIS helpers ----
SENTENCE = "!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5C"


def test_ais_known_sentence():
    bits = ais_bits_from_nmea(SENTENCE)
    assert len(bits) == 168
    body = np.packbits(bits).tobytes()
    frame = body + ax25_fcs(body)
    assert np.array_equal(ais_payload_bits(frame), bits)
    p = ais_position(frame)
    assert p["type"] == 1 and p["mmsi"] == 477553000 and p["heading"] == 181
    assert abs(p["longitude"] - -122.345833) < 1e-6 and abs(p["latitude"] - 47.582833) < 1e-6 and p["course"] == 51.0
    assert ais_nmea(frame, "B") == [SENTENCE]
    with pytest.raises(ValueError):
        ais_bits_from_nmea(SENTENCE[:-1] + "D")


def test_ais_long_and_odd_payloads():
    body = bytes(range(53))                                  # 424 bits: 71 characters, two fill bits, two sentences
    parts = ais_nmea(body + ax25_fcs(body), "A", seq=3)
    assert len(parts) == 2 and parts[0].startswith("!AIVDM,2,1,3,A,") and parts[1].startswith("!AIVDM,2,2,3,A,")
    assert parts[0].split(",")[6].startswith("0*") and parts[1].split(",")[6].startswith("2*")
    got = np.concatenate([ais_bits_from_nmea(parts[0]), ais_bits_from_nmea(parts[1])])
    assert np.array_equal(got, np.unpackbits(np.frombuffer(body, np.uint8)))
    other = bytes([5 << 2]) + bytes(20)                      # type 5: no position
    assert ais_position(other + ax25_fcs(other)) is None
    b18 = np.zeros(168, np.uint8)
    b18[:6] = [0, 1, 0, 0, 1, 0]
    b18[57:85] = [int(c) for c in format(int(round(4.5 * 600000)) & (2 ** 28 - 1), "028b")]
    b18[85:112] = [int(c) for c in format(int(round(-33.25 * 600000)) & (2 ** 27 - 1), "027b")]
    body = np.packbits(b18).tobytes()
    p = ais_position(body + ax25_fcs(body))
    assert p["type"] == 18 and abs(p["longitude"] - 4.5) < 1e-6 and abs(p["latitude"] + 33.25) < 1e-6
