"""Pin the saturating restatement of word-mode ksw_align2 (swsatlib.py, the specification of sw_long_kernel) to the compiled
reference where scores cross 32 767: -A 60..127 on 300-700 bp mates against windows holding a near-copy, with KSW_XSUBO |
KSW_XSTART as mem_matesw sets them.  Cases must reach the clamp (score 32 767) and tie for qe."""
import numpy as np
import pytest

import kswlib
import swsatlib
import widesw

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built (no reference sources here)")]


def _check(p, pool, tasks):
    ref = kswlib.ref_sw_batch(p, pool, tasks)
    got = swsatlib.sat_sw_batch(p, pool, tasks)
    for f in kswlib.SW_FIELDS:
        bad = np.nonzero(got[f] != ref[f])[0]
        assert len(bad) == 0, f"{len(bad)} differ in {f}; first task {tasks[bad[0]]} ref={ref[bad[0]]} restated={got[bad[0]]}"
    return ref


@pytest.mark.parametrize("a,b,seed", [(60, 90, 1), (90, 40, 2), (127, 127, 3)])
def test_restatement_matches_reference_past_the_clamp(a, b, seed):
    rng = np.random.default_rng(9300 + seed)
    p = kswlib.make_params(a=a, b=b, o_del=6 * a // 4, e_del=a // 4, o_ins=5 * a // 4, e_ins=a // 3)
    pool, tasks = widesw.gen_saturating(rng, p, 12)
    ref = _check(p, pool, tasks)
    assert (ref["score"] == swsatlib.SAT).sum() >= 4, "the clamp must be on the path"
    assert (ref["tb"] >= 0).any() and (ref["score2"] > 0).any()


def test_clamp_ties_for_qe_and_second_pass_stop():
    """Tandem repeats under -A 127: whole sets of columns hold 32 767 in the row that first reaches it."""
    rng = np.random.default_rng(9304)
    p = kswlib.make_params(a=127, b=60, o_del=100, e_del=20, o_ins=100, e_ins=20)
    pool, tasks = widesw.gen_tandem(rng, p, 6)
    mat = np.asarray(p["mat"], dtype=np.int64)
    ties = 0
    for tk in tasks:
        q, t = kswlib.sw_task_seqs(pool, tk)
        st = {}
        s, _, _, _, _ = swsatlib.sw_pass(q, t, mat, 127, 100, 20, 100, 20, 0x10000, 0x10000, st)
        ties += s == swsatlib.SAT and st["qe_ties"] > 1
    assert ties >= 3
    ref = _check(p, pool, tasks)
    assert (ref["tb"] >= 0).all()


def test_restatement_below_the_clamp_matches_oracle():
    """Where nothing saturates, the restatement is the oracle's recurrence (oracle/sw_oracle.c)."""
    rng = np.random.default_rng(9305)
    p = kswlib.make_params(a=4, b=6)
    pool, tasks = widesw.gen_saturating(rng, p, 10, qlen=(200, 900))
    orc, _ = kswlib.orc_sw_batch(p, pool, tasks)
    got = swsatlib.sat_sw_batch(p, pool, tasks)
    for f in kswlib.SW_FIELDS:
        assert (got[f] == orc[f]).all(), f
