"""Pin the oracle to the compiled reference at the edges of the integer domains the kernels accept: scaled and general
matrices with large entries, gap costs past 2^15 and 2^16 for extension and global alignment, and byte-mode Smith-Waterman
gap costs whose o+e wraps in ksw_u8's 8-bit lanes.  test_score_domain_gpu.py then holds the kernels to the oracle there."""
import numpy as np
import pytest

import domaingen as dg
import glbbin_ref as br
import kswgen
import kswlib

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built (no reference sources here)")]


def _check_ext(p, pool, tasks):
    ref = kswlib.ref_extend_batch(p, pool, tasks)
    orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    bad = np.nonzero(ref != orc)[0]
    assert len(bad) == 0, f"{len(bad)} differ; first task {tasks[bad[0]]} ref={ref[bad[0]]} orc={orc[bad[0]]}"
    return ref


def test_extend_scaled_scores_and_huge_gap_costs():
    rng = np.random.default_rng(9001)
    top = 0
    for p in dg.ext_edge_param_sets(rng):
        pool, tasks = dg.gen_ext_edges(rng, p, per=4, early_indel=int(p["o_del"]) > 30000 or int(p["e_del"]) > 30000)
        mx = dg.max_mat(p)
        assert ((np.maximum(tasks["h0"], 0) + tasks["qlen"].astype(np.int64) * mx) == dg.LIMIT).any()
        top = max(top, int(_check_ext(p, pool, tasks)["score"].max()))
    assert top > 30000  # the scores really reach the top of the accepted range


def test_extend_long_query_at_the_limit():
    rng = np.random.default_rng(9002)
    p = kswlib.make_params(a=3, b=4, o_del=9, e_del=3, o_ins=9, e_ins=3)
    pool, tasks = dg.gen_ext_edges(rng, p, qlens=(10000,), per=2, long_q=10666)
    assert tasks["qlen"].max() == 10666
    _check_ext(p, pool, tasks)


def _check_glb(p, pool, tasks):
    ref, rc = kswlib.ref_global_batch(p, pool, tasks)
    orc, oc = kswlib.orc_global_batch(p, pool, tasks)
    bad = np.nonzero(ref != orc)[0]
    assert len(bad) == 0, f"first task {tasks[bad[0]]} ref={ref[bad[0]]} orc={orc[bad[0]]}"
    for a, b in zip(rc, oc):
        assert np.array_equal(a, b)
    return ref


def test_global_scaled_scores_and_huge_gap_costs():
    rng = np.random.default_rng(9003)
    low = 0
    for p in [kswlib.make_params(a=127, b=127, o_del=1000, e_del=127, o_ins=900, e_ins=100),
              kswlib.make_params(a=64, mat=dg.big_matrix(rng, 64), o_del=300, e_del=30, o_ins=200, e_ins=40),
              kswlib.make_params(o_del=70000, e_del=1, o_ins=6, e_ins=1), kswlib.make_params(o_del=6, e_del=1, o_ins=65535, e_ins=2),
              kswlib.make_params(o_del=0, e_del=65537, o_ins=0, e_ins=65537), kswlib.make_params(o_del=40000, e_del=30000, o_ins=6, e_ins=1)]:
        pool, tasks, _ = dg.gen_glb_deep(rng, lens=(60, 300), per=3)
        low = min(low, int(_check_glb(p, pool, tasks)["score"].min()))
    assert low < -1_000_000


def test_global_routing_edges():
    rng = np.random.default_rng(9004)
    p = kswlib.make_params(a=5, b=20, o_del=30, e_del=1, o_ins=40, e_ins=1)
    pool, tasks, _ = dg.gen_glb_worst_edges(rng, p)
    _check_glb(p, pool, tasks)
    pool, tasks, _ = dg.gen_glb_shape_edges(rng)
    _check_glb(kswlib.make_params(), pool, tasks)


# ---- global: real scores across the lane kernels' 16-bit domain (domaingen's families) --------------------------------------------
# Besides pinning the oracle to the reference, each case asserts what test_score_domain_gpu.py relies on: which of the dispatcher's
# lane bins (glbbin_ref.expected_bins on the tasks' own bands) the family's deep scores reach, from the REFERENCE's scores.

def _family(batches):
    """Reference == oracle on every batch; returns the reference scores and the bins of all tasks (own bands, every bin switched on)."""
    scores, bins = [], []
    for label, p, (pool, tasks, _) in batches:
        scores.append(_check_glb(p, pool, tasks)["score"])
        bins.append(br.expected_bins(p, pool, tasks, narrow=False)[0])
        assert np.isin(bins[-1], dg.GLB_LANE_BINS).all(), label
    return np.concatenate(scores).astype(np.int64), np.concatenate(bins)


def _deep(scores, bins, b, at=-8192):
    """Real scores (not MINUS_INF) of bin b at or below `at`."""
    return int(((bins == b) & (scores <= at) & (scores > dg.MINUS_INF)).sum())


def test_global_deep_negative_equal_lengths():
    """All-mismatch pairs at own bands 0..15: down to -11129, and at least three real scores <= -8192 in each of bins 6, 7 and 5."""
    scores, bins = _family(dg.gen_glb_deep_negative_equal(np.random.default_rng(9100)))
    for b in (6, 7, 5):
        assert _deep(scores, bins, b) >= 3, b
    assert scores[scores > dg.MINUS_INF].min() <= -11000 and (scores == dg.MINUS_INF).sum() >= 15  # (qlen - tlen = 3 at bands 0..2)


def test_global_threshold_of_half_the_sentinel():
    """-8128, -8192 and -8256 at band 0 (bin 6), and under gap opens of 1740 at bands 0, 5 (bin 7) and 12 (bin 5)."""
    scores, bins = _family(dg.gen_glb_threshold())
    assert scores.tolist() == [-8128, -8192, -8256] * 4 and bins.tolist() == [6] * 6 + [7] * 3 + [5] * 3


def test_global_deep_negative_unequal_lengths():
    """|qlen - tlen| of 16..63 at bands up to 63: bin 0 (<64>) down to -10036, bin 3 (<96>) to -9711, bin 1 (<128>) to -9407."""
    scores, bins = _family(dg.gen_glb_deep_negative_unequal(np.random.default_rng(9101)))
    low = {b: int(scores[bins == b].min()) for b in (0, 3, 1)}
    assert set(bins) == {0, 3, 1} and (scores > dg.MINUS_INF).all()
    assert low == {0: -10036, 3: -9711, 1: -9407}
    for b in (0, 3, 1):
        assert _deep(scores, bins, b) >= 3, b


def test_global_empty_targets():
    """tlen = 0: a real score <= -8192 in every lane bin, a genuine MINUS_INF (qlen = w + 1) in every lane bin, and 0 for qlen = 0."""
    batches = dg.gen_glb_empty_target(np.random.default_rng(9102))
    scores, bins = _family(batches)
    qlen = np.concatenate([b[2][1]["qlen"] for b in batches])
    w = np.concatenate([b[2][1]["w"] for b in batches])
    for b in dg.GLB_LANE_BINS:
        assert _deep(scores, bins, b) >= 1 and ((bins == b) & (scores == dg.MINUS_INF)).sum() >= 1, b
    assert ((scores == dg.MINUS_INF) == (qlen > w)).all() and (scores[qlen == 0] == 0).all() and (qlen == 0).sum() == 2


def test_global_deep_positive():
    """Identical sequences under a=127 and a=21: 10160 .. 11684, and 10000 or more in every lane bin."""
    scores, bins = _family(dg.gen_glb_deep_positive(np.random.default_rng(9103)))
    assert scores.min() == 10160 and scores.max() == 11684
    for b in dg.GLB_LANE_BINS:
        assert ((bins == b) & (scores >= 10000)).sum() >= 1, b


def test_global_extreme_gaps_on_the_exhaustive_set():
    """Gap extensions of 1150 and gap opens of 1999 + 2000 on every pair of up to five bases at every band up to 7."""
    batches = dg.gen_glb_extreme_gaps()
    assert [len(b[2][1]) for b in batches] == [26576] * 4 + [11216]
    scores, bins = _family(batches)
    assert set(bins) == {6, 7} and scores.min() == -5727 and (scores > dg.MINUS_INF).all()


def test_global_n_bases_on_a_general_matrix():
    """15 % N in the queries, 5 % more in the targets, distinct entries in the matrix's N row and N column."""
    batches = dg.gen_glb_n_bases(np.random.default_rng(9104))
    for _, p, (pool, tasks, _) in batches:
        m = np.asarray(p["mat"]).reshape(5, 5)
        assert len(set(m[4, :].tolist() + m[:4, 4].tolist())) == 9
        seqs = [kswlib.task_seqs(pool, t) for t in tasks]
        assert sum(int((q == 4).sum()) for q, _ in seqs) > 100 and sum(int((t == 4).sum()) for _, t in seqs) > 100
    scores, bins = _family(batches)
    assert set(bins) == {6, 7, 5}


def _check_sw(p, pool, tasks):
    ref = kswlib.ref_sw_batch(p, pool, tasks)
    orc, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=8)
    ok = orc["rsv"] == 0
    for f in kswlib.SW_FIELDS:
        bad = np.nonzero((ref[f] != orc[f]) & ok)[0]
        assert len(bad) == 0, f"{f}: {len(bad)} differ; first task {tasks[bad[0]]} ref={ref[bad[0]]} orc={orc[bad[0]]}"
    return ok


@pytest.mark.parametrize("gaps,wrap", dg.sw_gap_param_sets())
def test_sw_byte_mode_gap_costs(gaps, wrap):
    """ksw_u8 holds o+e in a byte: (128,128) acts as an open-and-extend cost of 0, (130,127) as 1."""
    rng = np.random.default_rng(9005 + sum(gaps))
    o_del, e_del, o_ins, e_ins = gaps
    p = kswlib.make_params(a=1, b=4, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins)
    assert dg.wraps(p) == wrap
    pool, tasks = kswgen.gen_sw_fuzz(rng, 400, p)
    byte = (tasks["xtra"] & kswlib.KSW_XBYTE) != 0
    ok = _check_sw(p, pool, tasks)
    assert (byte & ok).sum() > 150 and (~byte & ok).sum() > 100


def test_sw_scaled_scores_and_routing_edges():
    rng = np.random.default_rng(9006)
    for p in [kswlib.make_params(a=1, b=4), kswlib.make_params(a=2, b=4), kswlib.make_params(a=3, b=5, o_del=20, e_del=5, o_ins=30, e_ins=3),
              kswlib.make_params(a=127, b=127, o_del=200, e_del=55, o_ins=150, e_ins=100),
              kswlib.make_params(a=100, mat=dg.big_matrix(rng, 100), o_del=255, e_del=255, o_ins=255, e_ins=255)]:
        pool, tasks = dg.gen_sw_edges(rng, p, dg.sw_edge_cases(p), per=2)
        _check_sw(p, pool, tasks)


def test_sw_word_mode_at_the_score_limit():
    """qlen*max(mat) = 31999, the largest product bmh_sw_batch accepts."""
    rng = np.random.default_rng(9007)
    p = kswlib.make_params(a=11, b=20, o_del=40, e_del=10, o_ins=40, e_ins=10)
    pool, tasks = dg.gen_sw_edges(rng, p, [(2909, dg.X_START), (2909, 0)], per=1)
    assert (tasks["qlen"].astype(int) * 11 == 31999).all()
    _check_sw(p, pool, tasks)
