"""Pin the oracle to the compiled reference where the wide extension kernel works and test_score_domain_cpu.py stops (32000):
ksw_extend2 with h0 + qlen*max(mat) from 32001 to millions, a = 1 on queries of 14 k, 40 k and 65 535 columns, -A 10 on 4 kb, and
gap costs e = 16384...65535 and o+e = 70000; then the per-seed record (mem_chain2aln) on long reads at -A 1 and -A 10 against the
reference's own mem_chain2aln.  test_wide_ext_gpu.py holds the int32 kernel to the oracle there."""
import os
import tempfile

import numpy as np
import pytest

import domaingen as dg
import kswgen
import kswlib
import reflib
import widegen as wg

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built (no reference sources here)")]


def _check_ext(p, pool, tasks):
    ref = kswlib.ref_extend_batch(p, pool, tasks)
    orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    bad = np.nonzero(ref != orc)[0]
    assert len(bad) == 0, f"{len(bad)} differ; first task {tasks[bad[0]]} ref={ref[bad[0]]} orc={orc[bad[0]]}"
    return ref


def test_extend_scores_past_16_bits():
    rng = np.random.default_rng(9101)
    p = kswlib.make_params(a=5, b=20, o_del=30, e_del=3, o_ins=30, e_ins=3, zdrop=2000)
    specs = [(100, 31501), (100, 31502), (6201, 1000), (6202, 1000), (300, 3_000_000), (2000, 5_000_000), (9000, 16_000_000 - 45_000)]
    pool, tasks = wg.gen_ext(rng, p, specs)
    res = _check_ext(p, pool, tasks)
    assert (res["score"][4:] > 3_000_000).all() and all(wg.goes_wide(p, int(t["qlen"]), int(t["h0"])) for t in tasks)


def test_extend_long_queries_at_a1_and_a10():
    rng = np.random.default_rng(9102)
    p = kswlib.make_params(a=1, b=4)
    pool, tasks = wg.gen_ext(rng, p, [(14000, 100), (40000, 100), (65535, 100)], w=(20,), indel=0.0)
    assert (_check_ext(p, pool, tasks)["qle"] > 10000).all()
    p = kswlib.make_params(a=10, b=4, zdrop=1000)
    pool, tasks = wg.gen_ext(rng, p, [(4000, h) for h in (0, 50, 500, 3000)] + [(4096, 100)], w=(50, 100))
    assert _check_ext(p, pool, tasks)["score"].max() > 32000


def test_extend_gap_costs_past_16_bits():
    rng = np.random.default_rng(9103)
    for g in wg.WIDE_GAP_SETS:
        p = kswlib.make_params(a=2, b=4, zdrop=100, **g)
        assert not dg.ext_gaps_accepted(p)
        pool, tasks = wg.gen_ext(rng, p, [(q, h) for q in (30, 200, 700) for h in (0, 50, 3000)], w=(5, 50), indel=0.02)
        _check_ext(p, pool, tasks)


@pytest.mark.skipif(not reflib.have_ref_bwa(), reason="oracle/_ref not built")
def test_seed_record_on_long_reads_matches_reference_chain2aln():
    rng = np.random.default_rng(9104)
    tmp = tempfile.mkdtemp(prefix="bmh_wide_")
    genome = kswgen.rand_seq(rng, 120000)
    fa = os.path.join(tmp, "g.fa")
    reflib.write_fasta(fa, "g", genome)
    reflib.build_index(fa)
    idx = reflib.lib().bwa_idx_load(fa.encode(), 7)
    l_pac, pac = reflib.pac_of(idx)
    n = 0
    for kw, lens in ((dict(a=1, b=4), (33000, 40000)), (dict(a=10, b=40, o_del=60, e_del=10, o_ins=60, e_ins=10), (4000, 4200))):
        p = kswlib.make_params(zdrop=100 * kw["a"], **kw)
        reads = wg.long_reads(rng, genome, 4, lens)
        chains, regs = reflib.chains_and_regs(idx, reflib.opt_from_params(p), reads)
        got = kswlib.orc_chain2aln_reads(p, l_pac, pac, reads, chains)
        for r, (a, b) in enumerate(zip(got, regs)):
            assert len(a) == len(b) and (a == b).all(), f"{kw} read {r}: {a} vs {b}"
            n += len(b)
        assert all(len(r) * kw["a"] > 32000 for r in reads)  # refused by the default context's seed bound
    assert n >= 8
