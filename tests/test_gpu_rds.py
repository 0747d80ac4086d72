"""The RDS decoder bank (kq_rds_*, ka9q_sdr_amd/csrc/kq_rds.hip) on the GPU: against the float64 model of tests/rds_model.py
from host and device memory, bit for bit against itself under other call splits and other slots, a slot set mid-stream,
sync lost and found again, and a loopback from a ModBank station through a receiver bank's flat FM channel.

The bank gives no bits, only what they make: the test holds the group records (every information word stored while in
sync, good or not, its ok bit, and the bit count at the group's end), the per-call counts and the per-frame sync flag and
block counters equal to the model's.  One differing bit after sync changes a word, an ok bit or a counter."""
import functools

import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.rds import GROUP_DTYPE, STATUS_DTYPE, RdsBank, RdsStation, group_array, rds_params, status_array
import rds_model as rm
from test_rds_model import make_groups, samples, sent

pytestmark = pytest.mark.gpu

DEV_HZ = 75000.0
# Measured on an MI355X over the parity rows below (worst of all slots), and the bars at 4 x that (float32 transform rounding
# moves by a small factor with size and content): z over all the samples, phi and tau over every frame after the filter's
# fill-in.  The slot's first frames, those of the fill-in (rm.settle_frames, 2 to 4 here), are held to the ceiling itself,
# 1e-2 rad and 1e-2 bit, which no phi or tau bar may exceed: there z is down to 1e-4 of its later size while the
# transform's rounding stays what it is, so arg A and arg B, and with them phi and tau, move by that much more (the model
# with z perturbed by the measured z error gives up to 6e-4 rad and 4e-5 bit there); these frames' own figures have not
# been measured on the GPU, the test prints them.  Z_ABS is no measurement either: the bar of kq_wfm for the same
# transforms, in units of the composite's full scale 2 pi 75000 / Fc.
Z_REL_MEASURED, PHI_MEASURED, TAU_MEASURED = 4.43e-7, 1.97e-7, 4.30e-8      # relative RMS, rad, bit
Z_REL_BAR, PHI_BAR, TAU_BAR = 4 * Z_REL_MEASURED, 4 * PHI_MEASURED, 4 * TAU_MEASURED
PHI_FIRST_BAR, TAU_FIRST_BAR = 1e-2, 1e-2
Z_ABS = 2e-5


@functools.lru_cache(maxsize=None)
def _parts(Fc, n, key, count, eps, pilot):
    g = make_groups(count + 1, seed=key)
    p = rm.parts(n, Fc, rm.group_bits(g), eps=eps, pilot=pilot, seed=key)
    for v in p:
        v.setflags(write=False)
    return g, p


@functools.lru_cache(maxsize=None)
def _rows(Fc, L, S, seed, count=14):
    """S composites of `count` groups (and a further one that keeps the subcarrier keyed to the end): sample-clock error 0 and
    +-40 ppm, any subcarrier phase, pilot 0.1 or none, noise 0.003 .. 0.02 rad/sample, injection 0.03 .. 0.04.  Rows 6 apart
    share groups, pulse train and programme (the slow parts of the generator); phase, injection and noise differ"""
    rng = np.random.default_rng(seed)
    n = samples(Fc, L, count)
    comp, groups = [], []
    for s in range(S):
        g, p = _parts(Fc, n, 1000 * seed + s % 6, count, (0.0, 40e-6, -40e-6)[s % 3], (0.1, 0.0)[(s // 3) % 2])
        x = rm.combine(p, injection=rng.uniform(0.03, 0.04), theta=rng.uniform(0, 2 * np.pi), noise=rng.uniform(0.003, 0.02),
                       seed=seed * 77 + s)
        comp.append(x.astype(np.float32))
        groups.append(g)
    comp = np.array(comp)
    comp.setflags(write=False)
    return comp, groups


@functools.lru_cache(maxsize=None)
def _model(Fc, Dr, L, M, S, seed, row, start=0):
    comp, _ = _rows(Fc, L, S, seed)
    x = comp[row].astype(np.float64)
    x[:start] = 0.0
    return rm.RdsModel(Fc, Dr, L, M).decode(x, start=start)


def _records(model_groups):
    out = np.zeros(len(model_groups), GROUP_DTYPE)
    for k, (blk, ok, vb, bit) in enumerate(model_groups):
        out[k]["block"], out[k]["ok"], out[k]["version_b"], out[k]["bit"] = blk, ok, vb, bit
    return out


def _run(bank, comp, calls, device=False):
    """comp [rows][n] in calls of (samples, nblocks) -> per slot: groups (all calls' records in order), counts [calls],
    status [F], baseband [F Lr]"""
    S = bank.max_slots
    groups, counts, sts, zs = [[] for _ in range(S)], [], [], [[] for _ in range(S)]
    pos = 0
    for n, nb in calls:
        chunk = np.ascontiguousarray(comp[:, pos:pos + n], np.float32)
        pos += n
        if not device:
            g, c, st = bank.process(chunk, nb)
        else:
            F = bank.frames(n)
            cap = bank.max_groups(n)
            dc = torch.from_numpy(chunk).cuda()
            dg = torch.zeros((S, cap, 4), dtype=torch.int32, device="cuda")
            dn = torch.zeros((S,), dtype=torch.int32, device="cuda")
            ds = torch.zeros((S, max(F, 1), 6), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert bank.process_device(dc.data_ptr(), n, n // nb, n // nb, nb, dg.data_ptr(), cap, dn.data_ptr(), ds.data_ptr(),
                                       max(F, 1)) == F
            bank.sync()
            g, c, st = group_array(dg), dn.cpu().numpy().astype(np.uint32), status_array(ds[:, :F])
        counts.append(c)
        sts.append(st)
        for s in range(S):
            groups[s].append(g[s, :c[s]])
            if bank.active[s]:
                zs[s].append(bank.pull_baseband(s))
    return ([np.concatenate(g) for g in groups], np.array(counts).T, np.concatenate(sts, axis=1),
            [np.concatenate(z) if z else np.zeros(0, np.complex64) for z in zs])


def _bank(Fc, Dr, L, M, S, max_samples, sources):
    b = RdsBank(Fc, Dr, L, M, max_slots=S, max_samples=max_samples)
    b.active = [False] * S
    for s, src in sources.items():
        b.set(s, rds_params(source=src))
        b.active[s] = True
    return b


def _margin(r, settle):
    """the model's smallest |y| over the median, from bit `settle` (rm.settle_bits: the filter's fill-in, in which |y| starts
    from 0 in the model too) on"""
    soft = np.abs(r["soft"][settle:])
    return soft.min() / np.median(soft)


def _bars(zr, dphi, dtau, nf):
    """z, and phi and tau at every frame: the slot's first nf frames (rm.settle_frames: the filter's fill-in) under their
    own bar; -> the five figures"""
    assert max(PHI_BAR, TAU_BAR, PHI_FIRST_BAR, TAU_FIRST_BAR) <= 1e-2
    fig = [zr, dphi[nf:].max(), dtau[nf:].max(), dphi[:nf].max(), dtau[:nf].max()]
    print("   z %.3e, dphi %.3e, dtau %.3e; fill-in frames: dphi %.3e, dtau %.3e" % tuple(fig))
    assert fig[0] <= Z_REL_BAR and fig[1] <= PHI_BAR and fig[2] <= TAU_BAR and fig[3] <= PHI_FIRST_BAR and fig[4] <= TAU_FIRST_BAR
    return fig


def _compare(r, groups, counts, st, z, frames_per_call, Fc, f0=0):
    """one slot against its model result r, from frame f0 on; -> (z relative RMS error, worst |dphi| mod pi, worst |dtau|)"""
    want = _records(r["groups"])
    assert np.array_equal(groups, want), (groups, want)
    edges = f0 + np.cumsum([0] + list(frames_per_call))
    per_call = [int(np.sum((r["group_frame"] >= a) & (r["group_frame"] < b))) for a, b in zip(edges[:-1], edges[1:])]
    assert counts.tolist() == per_call
    for k in ("synced", "blocks_ok", "blocks_bad"):
        assert np.array_equal(st[k], r[k][f0:]), k
    Lr = len(r["z"]) // len(r["synced"])
    zm = r["z"][f0 * Lr:]
    err = np.sqrt(np.mean(np.abs(z - zm) ** 2))
    assert err <= Z_ABS * 2 * np.pi * DEV_HZ / Fc, err
    dphi = np.abs((st["phase"] - r["phase"][f0:] + np.pi / 2) % np.pi - np.pi / 2)
    dtau = np.abs(st["timing"] - r["timing"][f0:])
    assert np.allclose(st["level"], r["level"][f0:], rtol=1e-3, atol=1e-6)
    return err / np.sqrt(np.mean(np.abs(zm) ** 2)), dphi, dtau


PARITY = [(128000, 8, 512, 513, 1, False), (128000, 4, 256, 769, 3, True), (240000, 8, 1000, 1001, 3, False),
          (384000, 16, 2048, 2049, 64, True), (384000, 32, 2048, 2049, 1, False)]


@pytest.mark.parametrize("Fc,Dr,L,M,S,device", PARITY)
def test_parity_with_the_model(gpu, Fc, Dr, L, M, S, device):
    comp, sent_groups = _rows(Fc, L, S, seed=S + Dr)
    n = comp.shape[1]
    src = [(7 * s) % S for s in range(S)]       # slot s decodes row src[s]
    F = n // L
    per = -(-F // 3)                            # three calls of whole frames
    calls = [(min(per, F - k * per) * L, min(per, F - k * per)) for k in range(3)]
    bank = _bank(Fc, Dr, L, M, S, per * L, dict(enumerate(src)))
    groups, counts, st, z = _run(bank, comp, calls, device)
    bank.close()
    worst = np.zeros(5)
    ratio = 1.0
    for s in range(S):
        r = _model(Fc, Dr, L, M, S, S + Dr, src[s])
        ratio = min(ratio, _margin(r, rm.settle_bits(Fc, M)))
        full = [g for g in r["groups"] if g[1] == 15]
        assert [g[:3] for g in full][-13:] == sent(sent_groups[src[s]])[1:14]     # the model decodes what was sent
        zr, dphi, dtau = _compare(r, groups[s], counts[s], st[s], z[s], [c[1] for c in calls], Fc)
        worst = np.maximum(worst, _bars(zr, dphi, dtau, rm.settle_frames(Fc, L, M)))
    print("rds parity Fc=%d Dr=%d L=%d M=%d S=%d device=%d: margin %.2f, z relative RMS %.3e, |dphi| %.3e rad, |dtau| %.3e bit; "
          "fill-in frames |dphi| %.3e rad, |dtau| %.3e bit" % (Fc, Dr, L, M, S, device, ratio, *worst))
    assert ratio >= 0.1


def test_split_and_independence(gpu):
    Fc, Dr, L, M, S = 128000, 8, 512, 513, 3
    comp, _ = _rows(Fc, L, S, seed=5)
    n = comp.shape[1]
    F = n // L
    ref = _bank(Fc, Dr, L, M, S, n, {s: s for s in range(S)})
    want = _run(ref, comp, [(n, 1)])
    ref.close()
    assert all(len(g) >= 13 for g in want[0])
    a, b = 37 * 1000, 61 * 700                  # blocks of 1000 and 700 samples: neither divides nor is divided by L
    splits = ([(a, 37), (b, 61), (n - a - b, 1)], [(L, 1)] * F, [(5 * L + 130, 1), (n - 7 * L - 130, 2), (2 * L, 4)])
    for k, calls in enumerate(splits):
        assert sum(c[0] for c in calls) == n and all(c[0] % c[1] == 0 for c in calls)
        bk = _bank(Fc, Dr, L, M, S, n, {s: s for s in range(S)})
        got = _run(bk, comp, calls, device=(k == 1))
        bk.close()
        for s in range(S):
            assert np.array_equal(got[0][s], want[0][s]), (k, s)
            assert got[1][s].sum() == want[1][s].sum()
            assert np.array_equal(got[2][s], want[2][s]), (k, s)
            assert np.array_equal(got[3][s], want[3][s]), (k, s)
    # each slot alone (in another slot number) gives the bits it gave beside the others
    for s in range(S):
        bk = _bank(Fc, Dr, L, M, 4, n, {3: s})
        got = _run(bk, comp, [(n, 2)])
        bk.close()
        assert np.array_equal(got[0][3], want[0][s]) and np.array_equal(got[2][3], want[2][s]), s
        assert np.array_equal(got[3][3], want[3][s]), s


def test_slot_set_mid_stream(gpu):
    Fc, Dr, L, M = 128000, 8, 512, 513
    comp, _ = _rows(Fc, L, 2, seed=9)
    n = comp.shape[1]
    b = _bank(Fc, Dr, L, M, 2, n, {0: 0})
    first = 40 * L + 300                        # not on a frame boundary
    chunk = np.ascontiguousarray(comp[:, :first], np.float32)
    F = b.frames(first)
    cap = b.max_groups(first)
    g1 = np.full((2, cap), 0xFF, np.uint8).repeat(16, axis=1).view(GROUP_DTYPE)
    c1 = np.full(2, 0xFFFFFFFF, np.uint32)
    s1 = np.full((2, F * 24), 0xFF, np.uint8).view(STATUS_DTYPE)
    keep = (g1.copy(), s1.copy())
    assert b.lib.kq_rds_process(b.h, chunk.ctypes.data, first, first, first, 1, 0, g1.ctypes.data, cap, c1.ctypes.data,
                                s1.ctypes.data, F) == F
    b.n += first
    # nothing written for the slot before it was set
    assert c1[1] == 0xFFFFFFFF and g1[1].tobytes() == keep[0][1].tobytes() and s1[1].tobytes() == keep[1][1].tobytes()
    assert c1[0] <= cap and s1[0]["synced"][-1] == 1
    b.set(1, rds_params(source=1))              # cold start at stream index `first`
    b.active[1] = True
    rest = n - first
    calls = [(3 * L, 3), (rest - 3 * L, 1)]
    groups, counts, st, z = _run(b, comp[:, first:], calls)
    b.close()
    r = _model(Fc, Dr, L, M, 2, 9, 1, start=first)
    f0 = first // L
    ratio = _margin(r, rm.settle_bits(Fc, M, keyed=first - f0 * L))
    assert ratio >= 0.1 and len(r["groups"]) >= 8, ratio
    frames = [(first + 3 * L) // L - f0, n // L - (first + 3 * L) // L]
    zr, dphi, dtau = _compare(r, groups[1], counts[1], st[1], z[1], frames, Fc, f0=f0)
    print("rds mid-stream: margin %.2f" % ratio)
    _bars(zr, dphi, dtau, rm.settle_frames(Fc, L, M, keyed=first - f0 * L))


def test_sync_lost_and_found_again(gpu):
    Fc, Dr, L, M = 128000, 8, 512, 513
    g = make_groups(17, seed=31)
    n = samples(Fc, L, 16)
    bits = rm.group_bits(g)
    x = rm.composite(n, Fc, bits, injection=0.035, noise=0.01, seed=5)
    quiet = rm.composite(n, Fc, bits, injection=0.0, noise=0.01, seed=5)     # the same with the subcarrier removed
    a, b = int(0.45 * Fc), int(0.85 * Fc)                                   # for 0.4 s: 18 blocks, lose_after is 10
    x[a:b] = quiet[a:b]
    x = x.astype(np.float32)
    r = rm.RdsModel(Fc, Dr, L, M).decode(x)
    s = r["synced"]
    fa, fb = a // L, b // L
    assert s[fa - 1] == 1 and (s[fa:fb + 8] == 0).any() and s[-1] == 1      # the model's status shows both states
    # (no margin to ask in the gap: there the bits are noise.  The records, counters and flags must still agree: a bit that
    # differs there would have to make or break a checkword to show, and a noise word passes one in 2^10 / 5)
    F = n // L
    bank = _bank(Fc, Dr, L, M, 1, n, {0: 0})
    groups, counts, st, z = _run(bank, x[None, :], [(n, 1)])
    bank.close()
    full = [(tuple(int(v) for v in q["block"]), int(q["ok"]), int(q["version_b"])) for q in groups[0] if q["ok"] == 15]
    assert all(q in sent(g) for q in full) and sent(g)[2] in full and sent(g)[15] in full
    assert np.array_equal(st[0]["synced"], s)
    _compare(r, groups[0], counts[0], st[0], z[0], [F], Fc)


# ---- loopback: ModBank -> receiver Bank (flat FM) -> RdsBank.process_bank on the bank's stream -------------------------
FS, INTERP, LB, MB, DRX = 12288000, 32, 8192, 8193, 32
CH_BW = 150000.0
RDR, RL, RM = 16, 2048, 2049


def test_loopback_through_the_receiver(gpu):
    """One FM station with stereo programme, pilot and RDS; an AM channel beside the flat FM one makes the bank run each
    call's demodulators on its second stream.  The decode in place must read the finished plane: bit for bit what a twin
    bank makes of the same plane pulled to the host."""
    per_call, count = 64, 7
    La = LB // INTERP
    rate = FS // INTERP
    n = samples(rate, per_call * La, count) + per_call * La
    calls = n // (per_call * La)
    name = "KA9Q FM "
    g = [(0x54A8, 0 << 12 | 1 << 10 | 10 << 5 | (k % 4), 0xE000 + k, ord(name[2 * (k % 4)]) << 8 | ord(name[2 * (k % 4) + 1]))
         for k in range(count + 2)]               # 0A groups: PI, TP 1, PTY 10, segment k mod 4 of the name
    m = rm.composite(n, rate, rm.group_bits(g), injection=0.04, theta=0.7, noise=0.0, seed=3, deviation_hz=DEV_HZ)
    pcm = (m * rate / (2 * np.pi * DEV_HZ)).astype(np.float32)[None, :]      # the multiplex in units of full deviation
    mod = kq.ModBank(FS, LB, MB, INTERP, max_stations=1, max_blocks=per_call)
    rx = kq.Bank(FS, LB, MB, DRX, 2, per_call)
    mod.set_station(0, kq.station_config("fm", frequency=1.0e6, amplitude_dbfs=-20.0, deviation=DEV_HZ, low=-60000.0,
                                         high=60000.0))                      # band edges that pass 59.4 kHz
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_FM_DEMOD, low=-CH_BW, high=CH_BW, second_lo=-1.0e6, flat=1))
    rx.add_channel(kq.channel_config(demod_type=kq.KQ_AM_DEMOD, low=-5000.0, high=5000.0, second_lo=5.0e6))
    rds = RdsBank.beside(rx, RDR, RL, RM, max_slots=1)
    twin = RdsBank(rate, RDR, RL, RM, max_slots=1, max_samples=per_call * rx.olen)
    rds.set(0, rds_params(source=0))
    twin.set(0, rds_params(source=0))
    rng = np.random.default_rng(11)
    recs = []
    for c in range(calls):
        _, s16 = mod.process(pcm[:, c * per_call * La:(c + 1) * per_call * La], per_call)
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)   # receiver noise (see test_gpu_modulate)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        F, dg, dn, ds = rds.process_bank(rx)
        gr, cn, st = group_array(dg), dn.cpu().numpy().astype(np.uint32), status_array(ds)   # ordered after the decode
        plane = np.concatenate([rx.audio(0, b) for b in range(per_call)])[None, :]
        tg, tc, tst = twin.process(plane)
        assert np.array_equal(cn, tc) and np.array_equal(gr[0, :cn[0]], tg[0, :tc[0]]) and np.array_equal(st, tst), c
        recs.append(gr[0, :cn[0]].copy())
    for h in (mod, rx, rds, twin):
        h.close()
    recs = np.concatenate(recs)
    full = [tuple(int(v) for v in q["block"]) for q in recs if q["ok"] == 15]
    print("rds loopback: %d groups, %d with every block good" % (len(recs), len(full)))
    k0 = g.index(full[0])
    assert full == g[k0:k0 + len(full)] and k0 <= 1                # every group after the first is the one sent, in order
    assert len(full) - (k0 == 0) >= 4
    st = RdsStation().feed(recs)
    assert st.ps == "KA9Q FM " and st.pi == 0x54A8 and st.pty == 10 and st.tp == 1


def test_shared_rows_and_gaps_from_host_equal_device(gpu):
    """Slots {0, 1, 3, 6} of 8 on source rows {2, 0, 2, 1}: two slots share a row, the active list has gaps, and the blocks
    lie in rows wider than a block.  Two host-memory calls (distinct rows staged, planes copied back a run of slots at a
    time) give bit for bit what a twin bank gives from device memory, and leave everything else of the host buffers alone."""
    Fc, Dr, L, M = 128000, 8, 512, 513
    S, slots, nb, bl, pad = 8, {0: 2, 1: 0, 3: 2, 6: 1}, 4, 5000, 100
    n = nb * bl
    comp, _ = _rows(Fc, L, 3, seed=5)
    assert comp.shape[1] >= 2 * n
    host = _bank(Fc, Dr, L, M, S, n, slots)
    twin = _bank(Fc, Dr, L, M, S, n, slots)
    for c in range(2):
        buf = np.full((3, nb, bl + pad), np.nan, np.float32)
        buf[:, :, :bl] = comp[:, c * n:(c + 1) * n].reshape(3, nb, bl)
        F = host.frames(n)
        cap = host.max_groups(n)
        gw, sw = 16 * cap, 24 * F                            # bytes of a slot's row that the call writes
        assert F >= 2
        g, st = np.full((S, gw + 32), 0xFF, np.uint8), np.full((S, sw + 24), 0xFF, np.uint8)
        cn = np.full(S, 0xFFFFFFFF, np.uint32)
        assert host.lib.kq_rds_process(host.h, buf.ctypes.data, nb * (bl + pad), bl + pad, bl, nb, 0, g.ctypes.data,
                                       g.shape[1] // 16, cn.ctypes.data, st.ctypes.data, st.shape[1] // 24) == F
        host.n += n
        dbuf = torch.from_numpy(buf).cuda()
        dg, dst = torch.from_numpy(np.full_like(g, 0xFF)).cuda(), torch.from_numpy(np.full_like(st, 0xFF)).cuda()
        dcn = torch.from_numpy(np.full(S, -1, np.int32)).cuda()
        torch.cuda.synchronize()
        assert twin.process_device(dbuf.data_ptr(), nb * (bl + pad), bl + pad, bl, nb, dg.data_ptr(), g.shape[1] // 16,
                                   dcn.data_ptr(), dst.data_ptr(), st.shape[1] // 24) == F
        twin.sync()
        dg, dst, dcn = dg.cpu().numpy(), dst.cpu().numpy(), dcn.cpu().numpy().view(np.uint32)
        for s in range(S):
            if s in slots:
                assert cn[s] == dcn[s] and cn[s] <= cap, (c, s)
                assert np.array_equal(g[s, :gw], dg[s, :gw]) and np.array_equal(st[s, :sw], dst[s, :sw]), (c, s)
                assert np.array_equal(host.pull_baseband(s), twin.pull_baseband(s)), (c, s)
                assert st[s, :sw].view(STATUS_DTYPE)["level"].min() > 0, (c, s)
                assert (g[s, gw:] == 0xFF).all() and (st[s, sw:] == 0xFF).all(), (c, s)
            else:
                assert cn[s] == 0xFFFFFFFF and (g[s] == 0xFF).all() and (st[s] == 0xFF).all(), (c, s)
        # the slots that share row 2 decode the same samples
        assert np.array_equal(st[0, :sw], st[3, :sw]) and not np.array_equal(st[0, :sw], st[1, :sw])
    host.close()
    twin.close()
