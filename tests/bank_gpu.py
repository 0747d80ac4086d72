"""What the GPU tests of the PCM decoder banks (tests/test_gpu_{tone,cw,rtty,psk,acars,ale,dsc,fsk,pag}.py) do alike when
they hold a bank against its model, written once: a status record as a dict, the models' records after a call, the
comparison slot by slot, the cut points of a stream, a call from device memory with padded rows, and the status plane.
Each test file binds what is its own -- the status dtype, the name of its records, status_array -- with functools.partial.

pytest does not rewrite the asserts of a helper module, so every assert here carries what it compared."""
import numpy as np
import torch

import ka9q_sdr_amd as kq


def status_of(dtype, rec):
    return {k: rec[k].tolist() if rec[k].ndim else int(rec[k]) for k in dtype.names}


def snap_one(records, m, planes=()):
    """(status, what the model's methods named in `planes` give, its records): `records` names the model's list"""
    return (m.status(),) + tuple(getattr(m, p)() for p in planes) + (list(getattr(m, records)),)


def snap(records, models, planes=()):
    return [snap_one(records, m, planes) for m in models]


def check(status, record, bank, want, st, *planes, slots=None, what=None, seen=None):
    """want: per slot (status, a row of every plane, records) of the model, as snap() makes them.  status(rec): the
    record as the model states it; record: the name of the bank's pull ("event": bank.event(slot, index)).  seen: per slot
    the records already compared (arenas only grow between clears), so that a record is pulled once"""
    counts = bank.counts()
    for s in (range(len(want)) if slots is None else slots):
        model, rows, records = want[s][0], want[s][1:-1], want[s][-1]
        assert status(st[s]) == model, (what, s, status(st[s]), model)
        for plane, row in zip(planes, rows):
            assert [int(v) for v in plane[s]] == row, (what, s, [int(v) for v in plane[s]], row)
        assert int(counts[s]) == len(records), (what, s, int(counts[s]), len(records))
        k0 = seen[s] if seen is not None else 0
        got = [getattr(bank, record)(s, k) for k in range(k0, len(records))]
        assert got == records[k0:], (what, s, got, records[k0:])
        if seen is not None:
            seen[s] = len(records)


def chunks(n, sizes):
    """cut points: the sizes in turn, over and over"""
    at, k, out = 0, 0, []
    while at < n:
        m = min(sizes[k % len(sizes)], n - at)
        out.append((at, at + m))
        at += m
        k += 1
    return out


def device_call(status_array, bank, chunk, nblocks, st, fmt=kq.KQ_PCM_F32, pad=5, extra=()):
    """the chunk from device memory: nblocks blocks of block_len in rows of block_len + pad (NaN / junk in between); the
    status plane on the device; extra: what the bank's process_device takes behind the status stride"""
    rows, n = chunk.shape
    bl = n // nblocks
    if fmt == kq.KQ_PCM_S16BE:
        buf = np.full((rows, nblocks, bl + pad), 0x0080, np.int16)              # the word -32768, byte-swapped
        buf[:, :, :bl] = chunk.astype(">i2").view(np.int16).reshape(rows, nblocks, bl)
    else:
        buf = np.full((rows, nblocks, bl + pad), np.nan, np.float32)
        buf[:, :, :bl] = chunk.reshape(rows, nblocks, bl)
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    bank.process_device(t.data_ptr(), nblocks * (bl + pad), bl + pad, bl, nblocks, st.data_ptr(), 1, *extra, fmt=fmt)
    bank.sync()
    return status_array(st)


def plane(words, bank):
    return torch.zeros((bank.max_slots, words), dtype=torch.int32, device="cuda")
