"""The float64 model of the RDS decoder (tests/rds_model.py) against its own generator: checkwords and offsets, groups
decoded at the small geometries under sample-clock error, the version flag, sync loss and return.  No GPU."""
import numpy as np
import pytest

import rds_model as rm

SHAPES = [(128000, 8, 512, 513), (128000, 4, 256, 769), (240000, 8, 1000, 1001)]


def make_groups(count, seed):
    """random groups; every third is version B (the block at position 2 sent with offset C')"""
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.integers(0, 65536, 4)) + (int(g % 3 == 0),) for g in range(count)]


def samples(Fc, L, count):
    """whole frames that hold `count` groups and 40 bits more: the generator's lead, the filter's delay, the last frame"""
    return int((104 * count + 40) / rm.BIT_HZ * Fc) // L * L


def sent(groups):
    return [(tuple(g[:4]), 15, g[4]) for g in groups]


def got(result):
    return [(g[0], g[1], g[2]) for g in result["groups"]]


def test_crc10_and_offsets():
    assert rm.crc10(0) == 0
    assert rm.crc10(1) == 0x1B9                     # x^10 mod g = g - x^10
    assert rm.crc10(2) == 0x372                     # x^11: the same shifted, still below x^10
    assert rm.crc10(4) == 0x6E4 ^ 0x5B9             # x^12: shifted again it reaches x^10 and is reduced once
    rng = np.random.default_rng(0)
    for info in [0, 1, 0x8000, 0xFFFF] + [int(v) for v in rng.integers(0, 65536, 50)]:
        for name, off in rm.OFFSETS.items():
            w = rm.block(info, name)
            assert w >> 10 == info and w < 1 << 26
            assert rm.crc10(w >> 10) ^ (w & 0x3FF) == off
            assert rm.hit(w) == name                # a hit for its own offset and, the syndromes being distinct, no other
        assert rm.hit(info << 10 | rm.crc10(info)) is None   # no offset at all: syndrome 0
    assert len(set(rm.OFFSETS.values())) == 5
    assert [rm.POSITION[k] for k in ("A", "B", "C", "C'", "D")] == [0, 1, 2, 2, 3]


def test_machine_on_clean_bits():
    groups = make_groups(6, seed=2)
    bits = np.concatenate([[1, 0, 1, 1, 0], rm.group_bits(groups)])    # five stray bits first
    m = rm.decode_bits(bits)
    # sync is taken at the second block; the first group comes with A, B of it, then C and D as they arrive
    assert [(g[0], g[1], g[2]) for g in m.groups] == sent(groups)
    assert [g[3] for g in m.groups] == [5 + 104 * (k + 1) for k in range(6)]
    assert m.synced and m.ok_count == 24 and m.bad_count == 0


@pytest.mark.parametrize("eps", [0.0, 40e-6, -40e-6])
@pytest.mark.parametrize("Fc,Dr,L,M", SHAPES)
def test_model_decodes_generated_groups(Fc, Dr, L, M, eps):
    groups = make_groups(15, seed=1)       # 14 to decode; the 15th keeps the subcarrier keyed to the last sample
    n = samples(Fc, L, 14)
    x = rm.composite(n, Fc, rm.group_bits(groups), injection=0.03, eps=eps, theta=1.0, noise=0.02, seed=3)
    r = rm.RdsModel(Fc, Dr, L, M).decode(x.astype(np.float32))
    full = [g for g in got(r) if g[1] == 15]
    assert full[-13:] == sent(groups)[1:14], (len(full), r["synced"])  # every group from the second on, in order
    assert all(g in sent(groups) for g in full)
    vb = {g[0]: g[2] for g in full}
    assert all(vb[tuple(g[:4])] == g[4] for g in groups[1:14])          # version_b follows C'
    soft = np.abs(r["soft"][rm.settle_bits(Fc, M):])      # 7 or 8 bits: the filter's fill-in, where |y| starts from 0
    print("Fc %d Dr %d L %d M %d eps %+.0e: %d groups, smallest |y| %.2f of the median" % (
        Fc, Dr, L, M, eps, len(full), soft.min() / np.median(soft)))
    assert soft.min() >= 0.3 * np.median(soft)


def test_sync_is_lost_in_noise_and_returns():
    Fc, Dr, L, M = SHAPES[0]
    groups = make_groups(16, seed=4)
    n = int(1.41 * Fc) // L * L
    bits = rm.group_bits(groups)
    x = rm.composite(n, Fc, bits, injection=0.035, noise=0.01, seed=5)
    quiet = rm.composite(n, Fc, bits, injection=0.0, noise=0.01, seed=5)     # the same, subcarrier off
    a, b = int(0.45 * Fc), int(0.85 * Fc)                                   # 0.4 s: 18 blocks, lose_after is 10
    x[a:b] = quiet[a:b]
    r = rm.RdsModel(Fc, Dr, L, M).decode(x.astype(np.float32), lose_after=10)
    s = r["synced"]
    fa, fb = a // L, b // L
    assert s[fa - 1] == 1 and (s[fa:fb] == 0).any() and s[-1] == 1, s
    lost = fa + int(np.flatnonzero(s[fa:] == 0)[0])
    assert r["blocks_bad"][lost] >= 10
    full = [g for g in got(r) if g[1] == 15]
    assert all(g in sent(groups) for g in full)
    assert sent(groups)[-1] in full and sent(groups)[2] in full            # groups before the gap and after it
