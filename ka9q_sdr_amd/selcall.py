"""Tone signalling around the tone decoder bank (tone.py, kq_tone_*): the tone plans as data (DTMF, ZVEI1, CCIR; any other
table goes in the same way), the bank's settings for a plan, encoders that make test traffic, and readers that turn the
bank's events into keys and call sequences.  Plain Python and numpy; nothing here touches a GPU.
"""
import collections

import numpy as np

# freqs: Hz, the first group's tones, then the second's.  keys: with two groups keys[i0 * groups[1] + i1] is the key of
# symbol i0 | i1 << 8; with one group keys[i] that of symbol i.  tone_s: the shortest tone a sender makes.  block_s: the
# decision block, about a quarter of it.  repeat: the key that stands for "the digit before, again", or None.
Plan = collections.namedtuple("Plan", "name freqs groups keys tone_s block_s repeat")

DTMF = Plan("DTMF", (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0), (4, 4), "123A456B789C*0#D", 0.050, 0.01275,
            None)
ZVEI1 = Plan("ZVEI1", (1060.0, 1160.0, 1270.0, 1400.0, 1530.0, 1670.0, 1830.0, 2000.0, 2200.0, 2400.0, 2600.0), (11,),
             "1234567890E", 0.070, 0.0175, "E")
CCIR = Plan("CCIR", (1124.0, 1197.0, 1275.0, 1358.0, 1446.0, 1540.0, 1640.0, 1747.0, 1860.0, 1981.0, 2110.0), (11,),
            "1234567890E", 0.100, 0.025, "E")
PLANS = {p.name: p for p in (DTMF, ZVEI1, CCIR)}

Key = collections.namedtuple("Key", "key start_sample blocks")
Call = collections.namedtuple("Call", "digits start_sample")


def plan_config(plan, samprate, **over):
    """ToneBank's (and the model's) keywords for a plan at a sample rate: block_len = rint(block_s Fs) (102 at 8 kHz and 612
    at 48 kHz for DTMF), frac 16 with two groups and 64 with one, ratio 64 (a best tone 6 dB above the next), twist 160
    (10 dB), min_blocks 2, min_ms 16.  `over` replaces any of them."""
    c = dict(block_len=int(np.rint(plan.block_s * samprate)), freqs=tuple(plan.freqs), groups=tuple(plan.groups),
             frac=16 if len(plan.groups) == 2 else 64, ratio=64, twist=160, min_blocks=2, min_ms=16)
    c.update(over)
    return c


def symbol_key(plan, symbol):
    """the key of a symbol of the bank, or None for one outside the plan"""
    if symbol < 0:
        return None
    i0, i1 = symbol & 0xFF, symbol >> 8
    k = i0 * plan.groups[1] + i1 if len(plan.groups) == 2 else i0
    return plan.keys[k] if k < len(plan.keys) and (len(plan.groups) == 2 or i1 == 0) else None


def key_tones(plan, key):
    """the frequencies of a key: two with two groups, else one"""
    k = plan.keys.index(key)
    if len(plan.groups) == 2:
        return plan.freqs[k // plan.groups[1]], plan.freqs[plan.groups[0] + k % plan.groups[1]]
    return (plan.freqs[k],)


def _noise(x, ref_amp, noise_db, seed):
    """white Gaussian noise noise_db below the power of a tone of amplitude ref_amp"""
    if noise_db is None:
        return x
    sigma = ref_amp / np.sqrt(2.0) * 10.0 ** (-noise_db / 20.0)
    return x + np.random.default_rng(seed).normal(0.0, sigma, len(x))


def dtmf_encode(keys, samprate, on=0.050, off=0.050, twist_db=0.0, amp=0.25, lead=0.0, tail=None, ferr=0.0, noise_db=None,
                seed=0, plan=DTMF):
    """float32 audio of a key train: each key `on` seconds of its two tones, then `off` seconds of silence, after `lead`
    seconds and before `tail` (default: off).  amp: the low tone's amplitude; the high tone is twist_db above it.  ferr:
    the relative frequency error of each key's tones, one number or one per key.  noise_db: white noise that many dB
    below the low tone (None: none), from `seed`.  Key k begins at sample rint((lead + k (on + off)) Fs)."""
    Fs = float(samprate)
    tail = off if tail is None else tail
    ferr = np.broadcast_to(np.asarray(ferr, np.float64), (len(keys),))
    n = int(np.rint((lead + len(keys) * (on + off) + tail) * Fs))
    x = np.zeros(n, np.float64)
    hi = amp * 10.0 ** (twist_db / 20.0)
    for k, key in enumerate(keys):
        a = int(np.rint((lead + k * (on + off)) * Fs))
        t = np.arange(int(np.rint(on * Fs))) / Fs
        f0, f1 = (f * (1.0 + ferr[k]) for f in key_tones(plan, key))
        x[a:a + len(t)] = amp * np.sin(2 * np.pi * f0 * t) + hi * np.sin(2 * np.pi * f1 * t)
    return _noise(x, amp, noise_db, seed).astype(np.float32)


def sequence_keys(digits, plan):
    """the keys a sender keys for a digit string: a digit equal to the key before it goes out as the repeat key, so no two
    tones in a row are the same (111 is 1 E 1)"""
    out = []
    for d in digits:
        out.append(plan.repeat if out and plan.repeat and d == out[-1] else d)
    return "".join(out)


def sequence_encode(digits, samprate, plan=ZVEI1, tone_s=None, amp=0.25, lead=0.0, tail=None, ferr=0.0, noise_db=None,
                    seed=0):
    """float32 audio of one sequential call: the digits' tones end to end with continuous phase, tone_s seconds each (the
    plan's by default), repeated digits by the repeat tone; after `lead` seconds of silence and before `tail` (default: one
    tone).  ferr and noise_db as in dtmf_encode (noise against the tone's power)."""
    Fs = float(samprate)
    tone_s = plan.tone_s if tone_s is None else tone_s
    tail = tone_s if tail is None else tail
    keys = sequence_keys(digits, plan)
    per = int(np.rint(tone_s * Fs))
    f = np.repeat([key_tones(plan, k)[0] for k in keys], per) * (1.0 + ferr)
    ph = 2 * np.pi * np.cumsum(f) / Fs
    x = np.concatenate([np.zeros(int(np.rint(lead * Fs))), amp * np.sin(ph), np.zeros(int(np.rint(tail * Fs)))])
    return _noise(x, amp, noise_db, seed).astype(np.float32)


def _field(e, name):
    return int(e[name]) if not hasattr(e, name) else int(getattr(e, name))


def read_dtmf(events, block_len, plan=DTMF):
    """The keys of a slot's events (ToneBank.events or the model's: symbol, blocks, start_sample), in order, as Key(key,
    start_sample, blocks): runs of one symbol less than two blocks apart are one key (a block lost to noise inside a long
    key does not split it)."""
    out = []
    end = sym = None
    for e in events:
        s, start, blocks = _field(e, "symbol"), _field(e, "start_sample"), _field(e, "blocks")
        key = symbol_key(plan, s)
        if key is None:
            continue
        if out and s == sym and start - end < 2 * block_len:
            out[-1] = Key(key, out[-1].start_sample, (start - out[-1].start_sample) // block_len + blocks)
        else:
            out.append(Key(key, start, blocks))
        sym, end = s, start + blocks * block_len
    return out


def read_sequence(events, block_len, plan=ZVEI1):
    """The sequential calls among a slot's events, as Call(digits, start_sample): tones less than two blocks apart belong
    to one call, and the repeat tone reads as the digit before it (at the head of a call it stays as it is)."""
    calls = []
    end = None
    for e in events:
        s, start, blocks = _field(e, "symbol"), _field(e, "start_sample"), _field(e, "blocks")
        key = symbol_key(plan, s)
        if key is None:
            continue
        if end is None or start - end >= 2 * block_len:
            calls.append([[], start])
        digits = calls[-1][0]
        digits.append(digits[-1] if key == plan.repeat and digits else key)
        end = start + blocks * block_len
    return [Call("".join(d), at) for d, at in calls]


__all__ = ["Plan", "DTMF", "ZVEI1", "CCIR", "PLANS", "Key", "Call", "plan_config", "symbol_key", "key_tones", "dtmf_encode",
           "sequence_keys", "sequence_encode", "read_dtmf", "read_sequence"]
