"""The three paths of the exact introsort (host/sort_exact.h) as hipcc compiles them: region_dedup_kernel's two sorts (per-lane
range stack of kDedupStk entries, csrc/chain2reg.hip) and chain_kernel's sort of chain weights (BMH_CC_STK entries, csrc/chain.hip),
on the inputs of tests/sortmodel.py that reach the combsort fallback -- its gap sequence in device double arithmetic, the 9/10 ->
11 rule, its trailing insertion sort, the hand-back into the range stack.  Expected outputs are the compiled reference's
(tests/golden/sort_paths_golden.npz); tests/test_sort_paths_cpu.py proves which path each input takes and checks the gcc build."""
import ctypes as C

import numpy as np
import pytest

import kswlib
import postgen
import sortmodel as sm
from __graft_entry__ import load_package
from test_chain_cpu import run_chain_reads
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return sm.fixture()


@pytest.fixture(scope="module")
def ctx():
    c = load_package().Context(0)
    yield c
    c.close()


def _host_dedup(v, level):
    lib = load_package().lib()
    lib.bmh_sort_and_dedup.restype = C.c_int
    lib.bmh_sort_and_dedup.argtypes = [C.c_int, C.c_void_p, C.c_float]
    a = np.array(v, dtype=kswlib.ALNREG, copy=True)
    n = lib.bmh_sort_and_dedup(len(a), a.ctypes.data_as(C.c_void_p), C.c_float(level))
    return a[:n].copy()


def test_region_fixture_at_every_level(ctx, fx):
    vecs = [v for _, v in fx["regs"]]
    for level in sm.LEVELS:
        got = ctx.sort_dedup_batch(vecs, level)
        assert len(got) == len(vecs)
        for (name, v), g, want in zip(fx["regs"], got, fx["reg_want"][level]):
            assert g.tobytes() == want.tobytes(), f"{name} at {level}: device keeps records {list(g['seedcov'][:40])}, reference {list(want['seedcov'][:40])}"
            assert g.tobytes() == _host_dedup(v, level).tobytes(), f"{name} at {level}: device and host differ"
        assert ctx.last_dedup_stats()[:2] == (sum(len(v) for v in vecs), sum(len(w) for w in fx["reg_want"][level]))


def test_answers_do_not_depend_on_the_neighbouring_lanes(ctx, fx):
    """Killer vectors interleaved with ordinary reads, then the same vectors in another order: lanes of one wave sit in combsort,
    quicksort and insertion sort at once, and every vector's neighbours change between the two batches."""
    rng = np.random.default_rng(20261018)
    plain = postgen.region_vectors(rng, 3 * len(fx["regs"]), 3_000_000)
    for level in (0.95, 1.0):
        vecs, want = [], []
        for ci, (name, v) in enumerate(fx["regs"]):
            vecs.append(v), want.append(fx["reg_want"][level][ci])
            for p in plain[3 * ci: 3 * ci + 3]:
                vecs.append(p), want.append(_host_dedup(p, level))
        got = ctx.sort_dedup_batch(vecs, level)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], [i for i, (g, w) in enumerate(zip(got, want)) if g.tobytes() != w.tobytes()][:10]
        order = rng.permutation(len(vecs))
        got = ctx.sort_dedup_batch([vecs[i] for i in order], level)
        assert [g.tobytes() for g in got] == [want[i].tobytes() for i in order], level
        assert ctx.last_dedup_stats()[:2] == (sum(len(v) for v in vecs), sum(len(w) for w in want))


@pytest.mark.parametrize("init_cap", [None, "16"])
def test_chain_fixture(fx, init_cap):
    """The device chainer over the synthetic seeding tables: the chains the reference's mem_chain_flt keeps, in its order, and what
    the host chainer gives.  The second run has BMH_CHAIN_INIT_CAP=16 in the environment while its context is made: that knob
    shrinks the first tables of the FUSED seeding + chaining calls only, bmh_chain_batch sizes its arena from the tables it is
    given, so for this entry point the run repeats the first one in a fresh context and grows nothing."""
    lib = load_package().lib()
    lib.bmh_chain_reads.restype = C.c_int
    ctx = _ctx_with({"BMH_CHAIN_INIT_CAP": init_cap} if init_cap else {})
    try:
        all_seeds = [s for _, s in fx["chains"]]
        for kw, want in zip(sm.CHAIN_OPTS, fx["chain_want"]):
            o = sm.chain_opt(kw)
            reads, calls, intvs, offs, sa_pos, sa_k = sm.chain_batch_tables(all_seeds, o)
            got = ctx.chain_batch(o, sm.CHAIN_L_PAC, reads, calls, intvs, offs, sa_pos)
            host = run_chain_reads(lib, o, sm.CHAIN_L_PAC, reads, calls, intvs, sa_k, sa_pos) if not init_cap else None
            for r, ((name, _), g, w) in enumerate(zip(fx["chains"], got, want)):
                assert all(len(c) == 1 for c in g), name
                g = np.concatenate(g) if g else np.zeros(0, kswlib.SEED)
                assert g.tobytes() == w.tobytes(), f"{name}: device keeps chains {list(g['rbeg'][:40] // sm._CH_STEP - 1)}, reference {list(w['rbeg'][:40] // sm._CH_STEP - 1)}"
                if host is not None:
                    assert g.tobytes() == np.concatenate(host[r]).tobytes(), f"{name}: device and host differ"
            st = ctx.chain_stats()
            assert (st["reads"], st["chains_in"], st["chains_out"]) == (len(all_seeds), sum(len(s) for s in all_seeds), sum(len(w) for w in want))
            assert st["seeds"] == st["chains_out"] and st["equal_keys"] == 0  # one seed per chain, no two at one position
    finally:
        ctx.close()
