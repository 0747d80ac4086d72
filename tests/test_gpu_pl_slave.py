"""The FM demodulator's PL slave, sample by sample: kq_bank_pull_pl_samples against the oracle's pl_filter->output_r in every
block, at every path the slave's transform can take (tests/pl_model.py CASES; tests/test_pl_model.py shows on the CPU that
this comparison sees a slave without butterflies, a time-reversed one, one that keeps the wrong samples and one without its
response, none of which `plfreq` notices reliably).

Bound: relative RMS over the run of (bank - oracle) <= 4 e_ref, e_ref being the distance of the oracle's samples from the
float64 model of the same case, computed from the oracle and the model alone.  Bank and oracle are both float32 chains of the
same transforms in a different order of operations; the factor 4 covers that and nothing more.

Measured on an MI355X (ratio to e_ref, de-emphasised / flat channel): see DESIGN_DIARY.md IV.11."""
import numpy as np
import pytest

import ka9q_sdr_amd as kq
import pl_model as pm
from common import bank_cfg, rel_rms
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pm.CASES, ids=pm.CASE_IDS)
def test_pl_samples_match_the_oracle_in_every_block(gpu, case):
    r = pm.case_reference(case)
    geom, plan, iq, nblocks, per_call = r["geom"], r["plan"], r["iq"], r["nblocks"], case[5]
    L = geom["L"]
    pl_n, pl_l = pm.pl_sizes(r["n_dec"], r["m_dec"])
    bank = kq.Bank(geom["samprate"], L, geom["M"], geom["D"], len(plan), per_call, fwd_mode=kq.KQ_FWD_AUTO)
    for p in plan:
        bank.add_channel(bank_cfg(p))
    got = [dict(audio=[], status=[], filt=[], pl=[]) for _ in plan]
    done = 0
    while done < nblocks:
        nb = min(per_call, nblocks - done)
        bank.push_iq(iq[done * L:(done + nb) * L])
        assert bank.process() == nb
        for c in range(len(plan)):
            for b in range(nb):
                got[c]["audio"].append(bank.audio(c, b))
                got[c]["status"].append(bank.status(c, b))
                got[c]["filt"].append(bank.filter_output(c, b))
                got[c]["pl"].append(bank.pl_samples(c, b))
        done += nb
    bank.close()
    e_ref, ratios = r["e_ref"], []
    for c in range(len(plan)):       # (printed before anything is asserted: a failing run still shows how far the samples are off)
        g, w = np.concatenate(got[c]["pl"]), np.concatenate(r["want"][c][3])
        assert len(g) == len(w) == nblocks * pl_l
        e = rel_rms(g, w)
        ratios.append(e / e_ref)
        print("%s channel %d: PL_N %d PL_L %d, bank - oracle %.3g = %.2f e_ref (e_ref %.3g)" % (case[0], c, pl_n, pl_l, e, e / e_ref, e_ref))
    _compare(plan, got, [w[:3] for w in r["want"]])
    assert not np.isnan(r["want"][1][1][-1]["plfreq"])       # three ring transforms: the tone has been read
    assert max(ratios) <= 4, (case[0], ratios, e_ref)


def test_pl_samples_are_refused_with_a_text(gpu):
    """the measurement off, a channel that is not FM, a buffer too small"""
    import ctypes as C
    g = dict(samprate=192000, L=1024, M=1025, D=4)
    fm = kq.channel_config(kq.KQ_FM_DEMOD, -8000.0, 8000.0)
    am = kq.channel_config(kq.KQ_AM_DEMOD, -5000.0, 5000.0)
    for pl_tone, ch, cap, text in ((False, 0, 64, "PL measurement is off"), (True, 1, 64, "not an FM channel"), (True, 0, 7, "too small")):
        bank = kq.Bank(g["samprate"], g["L"], g["M"], g["D"], 2, 2, pl_tone=pl_tone)
        bank.add_channel(fm)
        bank.add_channel(am)
        bank.push_iq(np.zeros(2 * g["L"], np.complex64))
        assert bank.process() == 2
        buf = np.zeros(64, np.float32)
        n = C.c_size_t(99)
        assert bank.lib.kq_bank_pull_pl_samples(bank.h, ch, 0, buf.ctypes.data, cap, C.byref(n)) == -1
        assert text in bank.lib.kq_last_error().decode() and n.value == 99
        if pl_tone:
            assert len(bank.pl_samples(0, 1)) == 8           # PL_L = 256 / 32
            with pytest.raises(kq.KqError):
                bank.pl_samples(0, 2)                        # no such block in the last call
        bank.close()
