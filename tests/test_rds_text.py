"""RdsStation (ka9q_sdr_amd/rds.py), the host-side reader of group records, on hand-built 0A / 0B / 2A / 2B groups.  No GPU."""
import numpy as np

from ka9q_sdr_amd.rds import GROUP_DTYPE, RdsStation

PI = 0x54A8


def block_b(gtype, version_b, tp, pty, low5):
    return gtype << 12 | version_b << 11 | tp << 10 | pty << 5 | low5


def two(s):
    return ord(s[0]) << 8 | ord(s[1])


def ps_groups(name, version_b=0, pty=10, tp=1):
    out = []
    for a in range(4):
        c = PI if version_b else 0xE0CD      # 0A: alternative frequencies; 0B: PI again, sent with C'
        out.append(((PI, block_b(0, version_b, tp, pty, a), c, two(name[2 * a:2 * a + 2])), 15, version_b))
    return out


def rt_groups(text, flag, version_b=0):
    per = 2 if version_b else 4
    text = text + "\r" if len(text) % per else text
    text = text.ljust(-(-len(text) // per) * per)
    out = []
    for a in range(len(text) // per):
        seg = text[per * a:per * a + per]
        b = block_b(2, version_b, 0, 5, flag << 4 | a)
        if version_b:
            out.append(((PI, b, PI, two(seg)), 15, 1))
        else:
            out.append(((PI, b, two(seg[:2]), two(seg[2:])), 15, 0))
    return out


def test_ps_name_pi_pty_tp_from_0a():
    st = RdsStation().feed(ps_groups("KA9Q FM "))
    assert st.ps == "KA9Q FM " and st.ps_complete
    assert (st.pi, st.pty, st.tp) == (PI, 10, 1)
    assert st.groups == 4


def test_ps_name_from_0b_and_out_of_order():
    g = ps_groups("RADIO-1!", version_b=1, pty=3, tp=0)
    st = RdsStation().feed([g[2], g[0]])
    assert st.ps == "RA  O-  " and not st.ps_complete
    st.feed([g[3], g[1]])
    assert st.ps == "RADIO-1!" and (st.pi, st.pty, st.tp) == (PI, 3, 0)


def test_only_blocks_with_their_ok_bit_are_used():
    g = ps_groups("GOODNAME")
    bad = ps_groups("XXXXXXXX")
    st = RdsStation()
    st.feed([(b[0], 0b0111, 0) for b in bad])           # block D failed: no characters
    assert st.ps == " " * 8 and st.pi == PI and st.pty == 10
    st.feed([(b[0], 0b1101, 0) for b in bad])           # block B failed: nowhere to put D
    assert st.ps == " " * 8
    st.feed([((0x1111,) + g[0][0][1:], 0b1110, 0)])     # block A failed: PI stays
    assert st.pi == PI and st.ps == "GO      "
    st.feed(g)
    assert st.ps == "GOODNAME"
    half = rt_groups("ABCDEFGH", 0)
    st.feed([(half[0][0], 0b1011, 0), (half[1][0], 0b0111, 0)])     # C of the first, D of the second lost
    assert st.radiotext == "  CDEF"


def test_radiotext_2a_with_flag_clearing():
    st = RdsStation().feed(rt_groups("Now playing: a long title", 0))
    assert st.radiotext == "Now playing: a long title"      # 25 characters: ended by 0x0D
    st.feed(rt_groups("Short", 0)[:1])                      # same flag: written over the old text
    assert st.radiotext == "Shorplaying: a long title"
    st.feed(rt_groups("Next", 1))                           # the flag toggled: cleared first
    assert st.radiotext == "Next"
    st.feed(rt_groups("Again", 1)[1:])
    assert st.radiotext == "Nextn"


def test_radiotext_2b():
    st = RdsStation().feed(rt_groups("2B carries two per group", 0, version_b=1))
    assert st.radiotext == "2B carries two per group"
    st.feed(rt_groups("odd", 1, version_b=1))
    assert st.radiotext == "odd"


def test_unprintable_characters_and_record_arrays():
    g = ps_groups("AB\x07\xe9 ~\x7f\x1f")
    rec = np.zeros(4, GROUP_DTYPE)
    for k, (blk, ok, vb) in enumerate(g):
        rec[k]["block"], rec[k]["ok"], rec[k]["version_b"] = blk, ok, vb
    st = RdsStation().feed(rec)
    assert st.ps == "AB?? ~??"
