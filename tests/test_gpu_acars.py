"""The ACARS decoder bank (kq_acars_*, ka9q_sdr_amd/csrc/kq_acars.hip) on the GPU against the integer model of
tests/acars_model.py: the records (bytes, length, flags, parity_errors, sync_sample, end_sample, the sync metric's two
terms, |R|^2), the arena counts and every field of the status record equal after every call, with no tolerance anywhere.
At 12 000 Hz (5 samples per bit, the shortest history) and at 39 062.5 Hz, on 9 slots (three workgroups of k_acars, the
last with one wave live): two share a row, one reads noise alone, one an inverted signal, the others senders with their
own delay, clock error, start phase and noise, one of them with blocks whose characters were spoilt on the way; from host and device memory, float and big-endian int16 input, padded rows,
in calls of 1, 80 and 4096 samples with a cut inside the sync's look-ahead and one inside the block check; with a slot set,
replaced and removed while a block is open, reset, a full arena, 4096 slots of which the last alone is set, and at 96 000
Hz (40 samples per bit, the longest history and filter, two waves to a workgroup) one block of 220 characters.  The model
runs on the bank's own taps, so nothing in the comparison is floating point but the quantiser's one multiply.  The
traffic is what tests/test_acars_model.py shows the model to decode."""
import functools

import numpy as np
import pytest
import torch

import acars_model as am
import bank_gpu
import ka9q_sdr_amd as kq
from ka9q_sdr_amd import arinc618
from ka9q_sdr_amd.acars import STATUS_DTYPE, STATUS_WORDS, AcarsBank, acars_params, status_array

pytestmark = pytest.mark.gpu

AMP = 0.3
LONG = "".join(chr(32 + (7 * i) % 95) for i in range(220))


def _traffic(kind):
    """the blocks a row carries"""
    if kind == 0:      # the 220-character block, an empty one
        return [arinc618.encode_block(text=LONG), arinc618.encode_block(text=None, label="_d")]
    if kind == 1:      # an ETB + ETX pair back to back, and a short one
        return [arinc618.encode_block(text="M01AXX0123 first half " * 3, more=True, block_id="1"),
                arinc618.encode_block(text="and the rest", block_id="2"), arinc618.encode_block(text="REQ WX KJFK", label="5Z")]
    out = [arinc618.encode_block(text="POS N4012 W07401 FL%03d" % (300 + kind), address=".N%03dAB" % kind, block_id=str(kind % 10))
           for _ in range(3)]
    if kind == 4:      # the second with one character of bad parity, the third with four
        out[1], out[2] = _spoil(out[1], (20,)), _spoil(out[2], (15, 18, 21, 24))
    return out


def _spoil(block, where):
    b = bytearray(block)
    for i in where:
        b[i] ^= 0x04
    return bytes(b)


# slot s reads row ROW[s]; row r: (traffic kind or None for noise alone, delay, ppm, invert, start phase, Eb/N0 dB or None)
ROW = (0, 0, 1, 2, 3, 4, 5, 6, 7)
ROWS = ((0, 0.0, 0.0, False, 0.0, None), (1, 0.37, 100.0, True, 1.0, 12.0), (None, 0, 0, False, 0, None),
        (2, 0.8, -100.0, False, 2.0, 10.0), (3, 0.5, 50.0, False, 0.3, None), (1, 0.1, 0.0, False, 0.0, 14.0),
        (4, 0.0, -50.0, True, 0.0, None), (5, 0.25, 0.0, False, 4.0, 12.0))


@functools.lru_cache(maxsize=None)
def _rows(Fs):
    """([rows][n] float32, read-only, 1.1 s), the blocks sent per row"""
    n = int(1.1 * Fs)
    out, sent = np.zeros((len(ROWS), n), np.float32), []
    for r, (kind, delay, ppm, inv, ph, db) in enumerate(ROWS):
        rng = np.random.default_rng(40 + r)
        if kind is None:
            out[r] = rng.normal(0.0, 0.1, n)
            sent.append([])
            continue
        blocks = _traffic(kind)
        x = arinc618.modulate(blocks, Fs, amp=AMP, ppm=ppm, invert=inv, start_phase=ph, delay=delay, lead=31 + 17 * r,
                              gap=int(0.01 * Fs))[:n]
        out[r, :len(x)] = x
        if db is not None:
            out[r] += rng.normal(0.0, am.noise_sigma(AMP, db, Fs), n).astype(np.float32)
        sent.append(blocks)
    out.setflags(write=False)
    return out, sent


def _model(bank, **kw):
    return am.AcarsModel(bank.samprate, input_scale=bank.input_scale, sync_num=bank.sync_num, sync_den=bank.sync_den,
                         max_parity_errors=bank.max_parity_errors, max_block_bytes=bank.max_block_bytes,
                         max_blocks=bank.max_blocks, taps=bank.get_taps(), **kw)


_status = functools.partial(bank_gpu.status_of, STATUS_DTYPE)
_snap = functools.partial(bank_gpu.snap, "blocks")
_check = functools.partial(bank_gpu.check, _status, "block")
_device_call, _plane = functools.partial(bank_gpu.device_call, status_array), functools.partial(bank_gpu.plane, STATUS_WORDS)


def _cuts(n, sizes, special=()):
    """call boundaries: the sizes in turn, over and over, and a boundary at every sample of `special`"""
    special = sorted(set(c for c in special if 0 < c < n))
    at, k, out = 0, 0, []
    while at < n:
        b = min(at + sizes[k % len(sizes)], n)
        nxt = [c for c in special if at < c < b]
        if nxt:
            b = nxt[0]
        else:
            k += 1
        out.append((at, b))
        at = b
    return out


def _special(Fs):
    """cuts inside the look-ahead of row 0's first sync -- three samples on, with sample p + 1 the last to have arrived --
    and inside its first block's check, found with a model of its own"""
    x, _ = _rows(Fs)
    m = am.AcarsModel(Fs)
    m.feed(x[0])
    r, g = m.blocks[0], m.g
    assert r.flags & am.GOOD and g.w >= 4
    mid = r.end_sample - int(8 * Fs / 2400.0)
    return [r.sync_sample + 2, r.sync_sample + 3, r.sync_sample + 4, mid, mid + 1, mid + g.w + 3]


@pytest.mark.parametrize("Fs", [12000.0, 39062.5])
def test_parity_from_host_and_device_memory(gpu, Fs):
    x, sent = _rows(Fs)
    n = x.shape[1]
    S = len(ROW)
    cuts = _cuts(n, (1, 80, 4096, 1, 1, 331), _special(Fs))
    assert {1, 80, 4096} <= {b - a for a, b in cuts}
    want = None
    for device in (False, True):
        bank = AcarsBank(Fs, S, 4096)
        for s, r in enumerate(ROW):
            bank.set(s, acars_params(source=r))
        if want is None:                                     # the models' records after every call, made once
            models, want = [_model(bank) for _ in range(S)], []
            g = models[0].g
            assert bank.get_slot(3) == (2, g.inc, g.FL, g.w, g.e, g.tb, g.H, bank.get_slot(0).piece)
            for a, b in cuts:
                for m, r in zip(models, ROW):
                    m.feed(x[r, a:b])
                want.append(_snap(models))
        st_t, seen = _plane(bank), [0] * S
        for (a, b), w in zip(cuts, want):
            nblocks = 4 if (b - a) % 4 == 0 else 1
            st = _device_call(bank, x[:, a:b], nblocks, st_t) if device else bank.process(x[:, a:b], nblocks)
            _check(bank, w, st, what=(device, a, b), seen=seen)
        if device:
            read = arinc618.read_blocks(bank)
            assert [(s, rec) for s, rec, _ in read] == [(s, rec) for s, m in enumerate(models) for rec in m.blocks]
            assert read[0][2].text == LONG and read[0][2].crc_ok and read[1][2].text == "" and read[1][2].label == "_d"
        bank.close()
    print("acars parity", Fs, [(m.syncs, m.blocks_good, m.blocks_bad, m.overruns, len(m.blocks)) for m in models])
    # what was sent is read: whole on the rows without noise, and nothing is filed from noise alone
    for s, (m, r) in enumerate(zip(models, ROW)):
        got = [rec.data for rec in m.blocks if rec.flags & am.GOOD]
        if ROWS[r][0] is None:
            assert not m.blocks and m.blocks_good == 0, s
        elif ROWS[r][0] == 4:
            bad = m.blocks[1]
            assert got == sent[r][:1] and len(m.blocks) == 2 and (m.blocks_bad, m.discarded) == (2, 1), s
            assert (bad.flags, bad.parity_errors, bad.data) == (0, 1, sent[r][1]) and arinc618.repair(bad.data, 1) == _spoil(bad.data, (20,))
            assert arinc618.parse(arinc618.repair(bad.data)).text == "POS N4012 W07401 FL304"
        elif ROWS[r][5] is None:
            assert got == sent[r], (s, got, sent[r])
        else:
            assert len(got) >= len(sent[r]) - 1 and all(b in sent[r] for b in got), s
    assert models[0].blocks == models[1].blocks and len(models[0].blocks) == 2      # the two slots on row 0
    assert models[2].blocks[0].flags & am.BY_ETB and not models[2].blocks[1].flags & am.BY_ETB


@pytest.mark.parametrize("device", [False, True])
def test_int16_input_and_clipping(gpu, device):
    """KQ_PCM_S16BE words, the word -32768 among them, and a float signal beyond the quantiser's range"""
    Fs = 12000.0
    x, sent = _rows(Fs)
    x = x[:2, :11000]
    loud = x * np.float32(5.0)
    assert (np.abs(loud[0]) * 32767 > 32767).mean() > 0.2
    words = am.quantise(x, 32767.0).astype(np.int16)
    words[:, 5:400:7] = -32768
    words[0, -3:] = -32768
    for data, fmt in ((loud, kq.KQ_PCM_F32), (words, kq.KQ_PCM_S16BE)):
        bank = AcarsBank(Fs, 2, 4096)
        for s in range(2):
            bank.set(s, source=s)
        models = [_model(bank) for _ in range(2)]
        st_t, seen = _plane(bank), [0, 0]
        for lo, hi in _cuts(x.shape[1], (1000, 4096)):
            st = _device_call(bank, data[:, lo:hi], 1, st_t, fmt) if device else bank.process(data[:, lo:hi], 1, fmt)
            for m, row in zip(models, data):
                m.feed(row[lo:hi], s16=fmt == kq.KQ_PCM_S16BE)
            _check(bank, _snap(models), st, what=(fmt, lo, hi), seen=seen)
        bank.close()
        assert models[0].blocks and models[0].blocks[0].data == sent[0][0], fmt       # clipped or not, the long block is read


def test_slot_lifecycle(gpu):
    """Slots set, replaced and removed while a block is open on their row; an arena of two blocks fills and counts what it
    drops; clear_blocks empties it and leaves the open block alone; a removed slot stops and keeps its arena; reset starts
    the grid over"""
    Fs = 12000.0
    x, sent = _rows(Fs)
    x = x[[4, 0]]                                            # three short blocks; the long one and the empty one
    n = x.shape[1]
    dry = am.AcarsModel(Fs)
    dry.feed(x[0])
    assert len(dry.blocks) == 3
    mid = [int(r.sync_sample + (r.end_sample - r.sync_sample) // 2) for r in dry.blocks]   # inside each block of row 0
    bank = AcarsBank(Fs, 4, n, max_blocks=2)
    src = {0: 0, 1: 1}
    for s, r in src.items():
        bank.set(s, source=r)
    models = {s: _model(bank) for s in src}

    def run(a, b, what):
        st = bank.process(x[:, a:b])
        for s, r in src.items():
            models[s].feed(x[r, a:b])
        _check(bank, {s: (m.status(), list(m.blocks)) for s, m in models.items()}, st, slots=list(src), what=what)
        return st

    st = run(0, mid[0], "open")
    assert int(st[0]["in_block"]) == 1 and int(st[1]["in_block"]) == 1 and not st[2].tobytes().strip(b"\0")
    # while both rows' blocks are open: slot 2 is set on row 0 (cold: it finds the second block first), slot 1 is replaced
    # (its open block goes, its row is now 0) and slot 3 is set and removed again
    bank.set(2, source=0)
    bank.set(1, source=0)
    bank.set(3, source=1)
    bank.remove(3)
    src[2], src[1] = 0, 0
    models[2], models[1] = _model(bank, start=mid[0]), _model(bank, start=mid[0])
    st = run(mid[0], mid[1], "set")
    assert int(st[0]["blocks_good"]) == 1 and int(st[2]["blocks_good"]) == 0 and int(st[2]["in_block"]) == 1
    assert not st[3].tobytes().strip(b"\0")
    # slot 0 is removed with its second block open: it stops, its arena stays
    bank.remove(0)
    kept = bank.blocks(0)
    del src[0], models[0]
    st = run(mid[1], n, "removed")
    assert not st[0].tobytes().strip(b"\0") and bank.blocks(0) == kept and len(kept) == 1
    assert int(st[2]["blocks_good"]) == 2 and [r.data for r in bank.blocks(2)] == sent[4][1:]
    # the arena of two is full: the same row again drops the rest; clear_blocks in between leaves the open block alone
    st = run(0, mid[0], "again")
    assert int(st[2]["in_block"]) == 1 and int(bank.counts()[2]) == 2
    st = run(mid[0], mid[2], "full")
    assert int(st[2]["dropped"]) == 2 and int(st[2]["blocks_good"]) == 4 and int(bank.counts()[2]) == 2
    bank.clear_blocks()
    for m in models.values():
        m.clear_blocks()
    assert not bank.counts().any()
    st = run(mid[2], n, "cleared")
    assert int(bank.counts()[2]) == 1 and bank.blocks(2)[0].data == sent[4][2]
    # reset: the grid starts over and every slot still set restarts cold
    bank.reset()
    models = {s: _model(bank) for s in src}
    st = run(0, n, "reset")
    assert int(st[1]["blocks_good"]) == 3 and bank.blocks(1)[0].sync_sample == dry.blocks[0].sync_sample
    bank.close()


def test_the_last_of_4096_slots(gpu):
    Fs = 12000.0
    x, sent = _rows(Fs)
    bank = AcarsBank(Fs, 4096, 4096, max_blocks=4)
    bank.set(4095, source=4)
    m = _model(bank)
    for a, b in _cuts(x.shape[1], (4096,)):
        st = bank.process(x[:, a:b])
        m.feed(x[4, a:b])
    assert _status(st[4095]) == m.status() and bank.blocks(4095) == m.blocks and len(m.blocks) == 3
    assert not st[:4095].tobytes().strip(b"\0") and int(bank.counts().sum()) == 3
    bank.close()


@pytest.mark.parametrize("device", [False, True])
def test_40_samples_per_bit(gpu, device):
    """96 000 Hz: FL = 80, w = 40, 1719 carried samples, two waves to a workgroup; one block of 220 characters on each of
    three slots (two workgroups), one of them 100 ppm fast and in noise"""
    Fs = 96000.0
    block = arinc618.encode_block(text=LONG)
    a = arinc618.modulate([block], Fs, amp=AMP, lead=100, delay=0.4)
    b = arinc618.modulate([block], Fs, amp=AMP, lead=977, ppm=100.0, invert=True, start_phase=1.0)
    n = len(b) + 500
    x = np.zeros((2, n), np.float32)
    x[0, :len(a)] = a
    x[1, :len(b)] = b
    x[1] += np.random.default_rng(9).normal(0.0, am.noise_sigma(AMP, 14.0, Fs), n).astype(np.float32)
    bank = AcarsBank(Fs, 3, 4096)
    for s, r in enumerate((0, 1, 0)):
        bank.set(s, source=r)
    assert bank.get_slot(0)[2:7] == (80, 40, 10, 10240, 1719)
    models = [_model(bank) for _ in range(3)]
    st_t, seen = _plane(bank), [0] * 3
    for lo, hi in _cuts(n, (4096, 80, 1, 4095)):
        st = _device_call(bank, x[:, lo:hi], 1, st_t) if device else bank.process(x[:, lo:hi])
        for m, r in zip(models, (0, 1, 0)):
            m.feed(x[r, lo:hi])
        _check(bank, _snap(models), st, what=(lo, hi), seen=seen)
    bank.close()
    for m in models:
        assert len(m.blocks) == 1 and m.blocks[0].data == block and m.blocks[0].flags == am.GOOD
