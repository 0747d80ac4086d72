"""The SAME integer model (tests/same_model.py) with the format helpers (ka9q_sdr_amd/eas.py) on the CPU: a noise-free alert
of three headers and three ends of message is read whole at three geometries, every header burst ends by the grammar and
the vote gives the text sent; the sync takes `sync_errs` wrong bits among its 48 and not one more; one flipped bit in the text
gives one bad or wrong byte that the vote mends; a flipped `+` leaves the burst to end by `lose` or `max_len`; a header of 31
locations is read whole; 60 s of noise and of a steady mark tone with the gate held open file nothing; and the noise and
clock-offset sweeps are printed.  tests/test_gpu_same.py holds the kernel equal to this model bit for bit, so what is shown
here holds for the bank.

Measured with this file (the model on a CPU, the defaults: snr 64, sync_errs 2, lose 3, max_len 248; an alert of three
headers of 42 bytes and three ends of message, white noise; printed by test_noise_sweep and test_clock_offset_sweep and copied
into include/ka9q_hip.h and DESIGN 4.29; nothing of it is asserted; four alerts a level, the pauses cut to 0.3 s), at
(48000, 8), (48000, 11) and (39062.5, 8): headers read with no wrong byte, of 12: 12, 12, 12 at 20, 16 and 14 dB Es/N0; 11,
10, 12 at 12 dB; 4, 4, 3 at 10 dB; none at 8 and 6 dB.  Alerts, of 4, whose vote is the text sent: 4, 4, 4 down to 12 dB; 4, 4,
3 at 10 dB; 1, 1, 2 at 8 dB; none at 6 dB.  Ends of message seen, of 12: all down to 10 dB; 10, 8, 12 at 8 dB; 3, 3, 5 at 6 dB.
Clock offsets of +-100, +-1000 and +-5000 ppm: 3 of 3 headers clean and 3 of 3 ends of message at every geometry.  Noise
alone and a steady mark tone, 60 s each with the gate forced open: 31223 and 31251 bits, nothing filed."""
import numpy as np
import pytest

import same_model as sm
from ka9q_sdr_amd import eas

AMP = 0.1
GEOMETRIES = [(48000.0, 8), (48000.0, 11), (39062.5, 8)]
TEXT = eas.header("WXR", "TOR", ["039173"], "0030", (159, 20, 15), "KCLE/NWS")
LONG = eas.header("EAS", "RWT", ["0%02d%03d" % (1 + k, 2 * k + 1) for k in range(31)], "0100", "0011234", "WXYZ-FM")


def _through_register(bits, **kw):
    """the bits through the model's steps 3 to 5 alone, the gate held open"""
    m = sm.SameModel(48000.0, 8, gate=False, **kw)
    for k, b in enumerate(bits):
        m.bit = int(b)
        m._bit(k, 0)
    return m


def _silence(n=40):
    return np.zeros(n, np.uint8)


def test_the_model_and_the_helpers_agree_on_the_constants():
    assert (sm.START, sm.BAD, sm.END) == (eas.START, eas.BAD, eas.END)
    assert (sm.COMPLETE, sm.LOST, sm.LENGTH) == (eas.COMPLETE, eas.LOST, eas.LENGTH)
    assert (sm.MARK, sm.SPACE, sm.BAUD) == (eas.MARK, eas.SPACE, eas.BAUD)
    assert (sm.PH, sm.PE) == (0xD5D55AC25AC2, 0xD5D572727272)
    # the patterns are the last 48 bits of a burst's preamble and first four bytes, in sending order
    for text, p in (("ZCZC", sm.PH), ("NNNN", sm.PE)):
        assert int("".join(str(b) for b in eas.burst(text)[-48:]), 2) == p


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
def test_a_noise_free_alert_is_read_whole(Fs, B):
    x = eas.modulate(TEXT, Fs, attention="weather", attention_seconds=1.0, amp=AMP)
    m = sm.SameModel(Fs, B).feed(x)
    bursts = eas.read(m.events)
    assert [b.kind for b in bursts] == ["Z"] * 3 + ["N"] * 3
    assert all(b.text == TEXT and b.reason == eas.COMPLETE and not b.bad and b.errs == 0 for b in bursts[:3])
    assert all(b.text == "NNNN" and b.errs == 0 for b in bursts[3:])
    assert (m.syncs, m.eoms, m.complete, m.lost, m.truncated, m.synced, m.dropped) == (3, 3, 3, 0, 0, 0, 0)
    assert m.nevents == 3 * (len(TEXT) - 4 + 2) + 3 and m.sync_sample == bursts[-1].start_sample
    assert eas.vote(bursts, Fs) == [eas.Alert(TEXT, 3, bursts[0].start_sample)]
    assert eas.parse(eas.vote(bursts, Fs)[0].text).event_name == "Tornado Warning"
    # the repeats start a burst and a second apart, and the burst takes its bits' time
    per = Fs / eas.BAUD
    want = (8 * (16 + len(TEXT)) * per + Fs)
    assert all(abs(b.start_sample - a.start_sample - want) <= per / 2 for a, b in zip(bursts[:2], bursts[1:3]))
    assert all(abs(b.end_sample - b.start_sample - 8 * (len(TEXT) - 4) * per) <= per / 2 for b in bursts[:3])


@pytest.mark.parametrize("sync_errs", [0, 2, 4])
def test_sync_takes_its_wrong_bits_and_not_one_more(sync_errs):
    b = eas.burst(TEXT)
    at = 8 * 16 + 32 - 48                                         # the first of the 48 sync bits
    rng = np.random.default_rng(sync_errs)
    for wrong in (sync_errs, sync_errs + 1):
        for _ in range(8):
            bits = b.copy()
            bits[at + rng.choice(48, wrong, replace=False)] ^= 1
            m = _through_register(np.concatenate([bits, _silence()]), sync_errs=sync_errs)
            if wrong <= sync_errs:
                got = eas.read(m.events)
                assert m.syncs == 1 and got[0].errs == wrong and got[0].text == TEXT and got[0].reason == eas.COMPLETE
            else:
                assert (m.syncs, m.nevents) == (0, 0)
    # an end of message likewise; it enters no sync
    e = eas.burst("NNNN")
    e[at + 5] ^= 1
    m = _through_register(np.concatenate([e, _silence()]), sync_errs=sync_errs)
    assert (m.eoms, m.synced, m.nevents) == ((1, 0, 1) if sync_errs else (0, 0, 0))


def _three(damage):
    """three bursts through the register, burst j with the bits damage[j] (of the text behind ZCZC) flipped"""
    out = []
    for flips in damage:
        bits = eas.burst(TEXT)
        for f in flips:
            bits[8 * 20 + f] ^= 1
        out += [bits, _silence(600)]
    return _through_register(np.concatenate(out))


@pytest.mark.parametrize("bit", [3, 7])
def test_one_flipped_bit_gives_one_wrong_or_bad_byte_and_the_vote_mends_it(bit):
    at = 10                                                        # a byte of the event code
    m = _three([[], [8 * at + bit], []])
    bursts = eas.read(m.events)
    assert len(bursts) == 3 and bursts[0].text == bursts[2].text == TEXT
    bad = bursts[1]
    differ = [k for k, (a, b) in enumerate(zip(bad.data, TEXT.encode())) if a != b]
    assert differ == [4 + at] and len(bad.data) == len(TEXT) and bad.reason == eas.COMPLETE
    assert bad.bad == ([4 + at] if bit == 7 else [])             # bit 7 set: outside 0x20..0x7E, filed with the BAD flag
    assert eas.vote(bursts, 48000.0) == [eas.Alert(TEXT, 3, bursts[0].start_sample)]


def test_the_vote_mends_disjoint_errors_in_all_three():
    m = _three([[8 * 3 + 1, 8 * 30 + 7], [8 * 9 + 2], [8 * 17 + 0, 8 * 18 + 6]])
    bursts = eas.read(m.events)
    assert len(bursts) == 3 and all(b.text != TEXT for b in bursts)
    assert eas.vote(bursts, 48000.0)[0].text == TEXT


@pytest.mark.parametrize("kw,reason", [(dict(), eas.LOST), (dict(lose=15), eas.LENGTH), (dict(lose=15, max_len=64), eas.LENGTH)])
def test_a_flipped_plus_ends_the_burst_by_lose_or_max_len(kw, reason):
    """`+` read as `*`: the dashes behind it do not count, the burst runs on into what follows -- here noise bits -- and ends
    by `lose` bad bytes in a row or, with `lose` out of reach, by max_len"""
    bits = eas.burst(TEXT)
    plus = TEXT.index("+")
    bits[8 * (16 + plus) + 0] ^= 1
    assert chr(ord("+") ^ 1) == "*"
    noise = np.random.default_rng(2).integers(0, 2, 8 * 300).astype(np.uint8)
    m = _through_register(np.concatenate([bits, noise]), **kw)
    b = eas.read(m.events)[0]
    assert b.reason == reason and b.reason != eas.COMPLETE and m.complete == 0
    assert b.text[:len(TEXT)] == TEXT[:plus] + "*" + TEXT[plus + 1:]
    if reason == eas.LENGTH:
        assert len(b.data) - 4 == m.max_len and m.truncated == 1
    else:
        assert m.lost == 1 and b.bad[-m.lose:] == list(range(len(b.data) - m.lose, len(b.data)))
    # ... and the vote over this burst and two whole ones is the text sent
    good = eas.read(_through_register(np.concatenate([eas.burst(TEXT), _silence()])).events)[0]
    assert eas.vote([good, b._replace(start_sample=good.start_sample + 90000), good._replace(start_sample=good.start_sample + 180000)],
                    48000.0)[0].text == TEXT


@pytest.mark.parametrize("Fs,B", GEOMETRIES[:1])
def test_a_header_of_31_locations_is_read_whole(Fs, B):
    assert len(LONG) == 4 + 4 + 4 + 31 * 7 + 5 + 8 + 10 and len(LONG) - 4 == 248
    x = eas.modulate(LONG, Fs, amp=AMP, eom=False, repeats=1)
    m = sm.SameModel(Fs, B).feed(x)
    b = eas.read(m.events)
    assert len(b) == 1 and b[0].text == LONG and b[0].reason == eas.COMPLETE and m.truncated == 0
    assert len(eas.parse(b[0].text).locations) == 31


SECONDS = 60.0


def test_noise_and_a_steady_tone_file_nothing():
    """60 s each with the gate forced open (snr 16, min_p 0, no warm-up): 31250 attempts on either pattern"""
    Fs, B = 48000.0, 8
    rng = np.random.default_rng(6)
    m = sm.SameModel(Fs, B, snr=16, min_p=0, warm=0)
    for _ in range(int(SECONDS)):
        m.feed(rng.normal(0.0, 0.1, int(Fs)).astype(np.float32))
    print("same noise alone, %g s, gate open: %d bits, syncs %d, eoms %d, events %d" % (SECONDS, len(m.bits), m.syncs, m.eoms, m.nevents))
    assert all(v for _, v in m.bits[1:]) and len(m.bits) > 31000
    assert (m.syncs, m.eoms, m.nevents, m.synced) == (0, 0, 0, 0)
    n = np.arange(int(SECONDS * Fs))
    x = (AMP * np.cos(2 * np.pi * eas.MARK / Fs * n)).astype(np.float32)
    m = sm.SameModel(Fs, B, snr=16, min_p=0, warm=0).feed(x)
    print("same steady mark, %g s, gate open: %d bits, syncs %d, eoms %d" % (SECONDS, len(m.bits), m.syncs, m.eoms))
    assert {b for b, _ in m.bits[10:]} == {1} and all(v for _, v in m.bits[1:]) and (m.syncs, m.eoms, m.nevents) == (0, 0, 0)


def test_call_boundaries_change_nothing():
    Fs, B = 48000.0, 8
    x = eas.modulate(TEXT, Fs, amp=AMP, eom=False, repeats=1, lead=0.05, tail=0.05)
    x = x + np.random.default_rng(4).normal(0.0, sm.noise_sigma(AMP, 14.0, Fs), len(x)).astype(np.float32)
    whole = sm.SameModel(Fs, B).feed(x)
    assert whole.syncs == 1 and whole.complete == 1
    for cut in (1, B - 1, B, B + 1, 9000):
        m = sm.SameModel(Fs, B)
        for at in range(0, len(x), cut):
            m.feed(x[at:at + cut])
        assert m.events == whole.events and m.status() == whole.status(), cut


def _clean_bursts(m):
    """header bursts read with no wrong byte, and ends of message seen"""
    b = eas.read(m.events)
    return sum(v.kind == "Z" and v.text == TEXT and v.reason == eas.COMPLETE for v in b), sum(v.kind == "N" for v in b)


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
def test_noise_sweep(Fs, B):
    """printed, not asserted: nobody has measured these.  Four alerts a level, each with noise of its own"""
    for db in (20, 16, 14, 12, 10, 8, 6):
        heads = eoms = voted = 0
        for seed in range(4):
            x = eas.modulate(TEXT, Fs, amp=AMP, gap=0.3, lead=0.05, tail=0.05)
            x = x + np.random.default_rng(100 + seed).normal(0.0, sm.noise_sigma(AMP, db, Fs), len(x)).astype(np.float32)
            m = sm.SameModel(Fs, B).feed(x)
            h, e = _clean_bursts(m)
            heads, eoms = heads + h, eoms + e
            voted += [a.text for a in eas.vote(eas.read(m.events), Fs)] == [TEXT]
        print("same noise", Fs, B, db, "dB: %d of 12 headers clean, %d of 12 ends of message, the vote right in %d of 4 alerts"
              % (heads, eoms, voted))


@pytest.mark.parametrize("Fs,B", GEOMETRIES)
def test_clock_offset_sweep(Fs, B):
    """printed, not asserted"""
    for ppm in (100, -100, 1000, -1000, 5000, -5000):
        m = sm.SameModel(Fs, B).feed(eas.modulate(TEXT, Fs, amp=AMP, ppm=ppm, lead=0.05, tail=0.05))
        h, e = _clean_bursts(m)
        print("same clock offset", Fs, B, "%+d ppm: %d of 3 headers clean, %d of 3 ends of message" % (ppm, h, e))


def test_widest_intermediates_stay_inside_the_header_bounds():
    Fs, B = 1024000.0, 256
    n = np.arange(20 * 8192)
    x = np.sign(np.cos(2 * np.pi * 1250.0 / Fs * n)).astype(np.float32)
    m = sm.SameModel(Fs, B, mark=1250.0, space=1500.0, baud=125.0).feed(x)
    wd = m.widest
    assert m.W == 32 and wd["acc"] < 1 << 38 and wd["red"] < 1 << 26 and wd["sum"] < 1 << 31 and wd["P"] < 1 << 63
