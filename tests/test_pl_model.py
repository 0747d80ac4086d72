"""The float64 model of the PL slave and tracker (tests/pl_model.py) against the oracle, and what a sample-level comparison
of the slave sees that `plfreq` does not.  CPU only.

For every case of pl_model.CASES: the oracle's PL samples (pl_filter->output_r after every block) against the model fed from
the oracle's own detected samples -- their relative RMS distance is e_ref, the float32 rounding of the oracle's transforms,
and the yardstick of the GPU test (tests/test_gpu_pl_slave.py holds the bank to 4 e_ref); the model's tracker reads the
oracle's plfreq in every block; and four wrong slaves each lie at least 100 e_ref from the oracle's samples."""
import numpy as np
import pytest

import pl_model as pm
from common import rel_rms


@pytest.mark.parametrize("case", pm.CASES, ids=pm.CASE_IDS)
def test_model_matches_the_oracle_and_the_mutants_do_not(case):
    r = pm.case_reference(case)
    pl_n, pl_l = pm.pl_sizes(r["n_dec"], r["m_dec"])
    oracle = np.concatenate(r["want"][1][3])
    assert len(oracle) == r["nblocks"] * pl_l and np.all(np.isfinite(oracle))
    # the de-emphasised channel's slave hangs off the same audio master (fm.c:219): the same samples
    assert np.array_equal(oracle, np.concatenate(r["want"][0][3]))
    e_ref = r["e_ref"]
    print("%s: PL_N %d PL_L %d, %d blocks, e_ref %.3g" % (case[0], pl_n, pl_l, r["nblocks"], e_ref))
    # float32 transforms of N_dec and PL_N points: a few 1e-7 (the PL band holds a small part of the window's energy, which
    # is where the rounding comes from); 1e-5 is the project's bar for any float output
    assert 0 < e_ref < 1e-5, e_ref
    tones = pm.pl_track(r["model"], r["dsamprate"])
    want = [s["plfreq"] for s in r["want"][1][1]]
    assert all((np.isnan(a) and np.isnan(b)) or a == b for a, b in zip(tones, want)), list(zip(tones, want))
    assert not np.isnan(want[-1])
    for m in pm.MUTANTS:
        d = rel_rms(pm.pl_slave(r["stream"], r["n_dec"], r["m_dec"], r["resp"], mutant=m).ravel(), oracle)
        print("    mutant %-14s %.3g = %.3g e_ref" % (m, d, d / e_ref))
        assert d >= 100 * e_ref, (m, d, e_ref)

