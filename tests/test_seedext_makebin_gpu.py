"""The fused per-seed record's two big rounds make their tasks and bin them in ONE pass (seed_left_make_bin /
seed_right_make_bin, seedext.hip; extend_binned_begin / _finish, extend_dispatch.hip): batches built for the edges of that pass,
through bmh_seedext_batch and bmh_seedext_batch_device, every record against the oracle's per-seed function bit for bit, and
the statistics counters against counts taken from the seed records on the host."""
import numpy as np
import pytest

import devcalls as dc
import kswgen
import kswlib
import widegen as wg
from __graft_entry__ import load_package
from test_device_entry_gpu import FORK_MIN_TASKS, _sync_code, _tg, concat_seeds, seed_flank
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

ENVS = {"auto": {}, "lane": {"BMH_EXT_SMALL": "0"}}  # small batches on one wave per task / every batch on the lane kernels


@pytest.fixture(scope="module", params=list(ENVS))
def ctx(request):
    c = _ctx_with(ENVS[request.param])
    yield c
    c.close()


def make_seeds(rng, specs, ctxlen=40, sub=0.02):
    """One seed per (L, qbeg, ln) in `specs`: a read of L bases, its window (the read with substitutions between `ctxlen`
    random bases on either side) and an exact seed read[qbeg:qbeg+ln] -- a left flank of qbeg and a right flank of
    L-qbeg-ln bases."""
    pb = kswgen.PoolBuilder(kswlib.SEED_TASK)
    for L, qbeg, ln in specs:
        read = kswgen.rand_seq(rng, L)
        mid = kswgen.mutate(rng, read, sub, 0.0, 0.0)
        mid[qbeg:qbeg + ln] = read[qbeg:qbeg + ln]
        win = np.concatenate([kswgen.rand_seq(rng, ctxlen), mid, kswgen.rand_seq(rng, ctxlen)])
        qo, to = pb.put(read), pb.put(win)
        pb.tasks.append((qo, to, L, qbeg, ln, ctxlen + qbeg, len(win), 0, 0))
    return pb.finish()


def host_counts(tasks):
    """(left tasks, right tasks) as the make-and-bin passes count them: seeds with a left flank, seeds with a right one."""
    return int((tasks["qbeg"] > 0).sum()), int((tasks["qbeg"] + tasks["len"] != tasks["l_query"]).sum())


def check(ctx, p, pool, tasks, what=""):
    """Both entry points on one batch: records exact, counters of the host-buffer call equal to the host's own counts."""
    ctx.set_params(p)
    want, _, calls = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    got = ctx.seedext_batch(pool, tasks)
    dc.assert_seed(got, want, tasks, what + "host buffers: ")
    st = ctx.seedext_stats()
    left, right = host_counts(tasks)
    assert st["seeds"] == len(tasks)
    assert (st["left_tasks"], st["right_tasks"]) == (left, right), f"{what}{st} against {left} left and {right} right tasks"
    assert left + st["left_retries"] + right + st["right_retries"] == calls == int(want["n_ext"].sum())
    ctx.set_qcap(max(int(seed_flank(tasks).max()), 1))
    s = dc.Seed(pool, tasks)
    s.run(ctx)
    ctx.sync()
    dc.assert_seed(s.result(), want, tasks, what + "device buffers: ")
    return want, st


def test_no_seed_has_the_flank(ctx):
    """every entry of a round is a sentinel and every bin is empty: no left flank anywhere, then no right flank anywhere,
    then neither (the seed covers the read)"""
    rng = np.random.default_rng(7100)
    p = kswlib.make_params()
    n = 700
    Ls = rng.integers(60, 200, n)
    lns = rng.integers(19, 40, n)
    for name, specs in (("no left", [(int(L), 0, int(ln)) for L, ln in zip(Ls, lns)]),
                        ("no right", [(int(L), int(L - ln), int(ln)) for L, ln in zip(Ls, lns)]),
                        ("neither", [(int(L), 0, int(L)) for L in Ls])):
        pool, tasks = make_seeds(rng, specs)
        for _ in range(2):  # the second call runs with the first one's bin-size hints (all zero for the empty round)
            _, st = check(ctx, p, pool, tasks, name + ": ")
        assert (st["left_tasks"] == 0) == (name != "no right") and (st["right_tasks"] == 0) == (name != "no left")


@pytest.mark.parametrize("n", [1, 63, 65, 1037, 3 * 1024 + 1, 5003])
def test_batch_sizes_off_the_grain(ctx, n):
    """one seed; sizes that are no multiple of the wave, of the block, or of the per-block range of the pass"""
    p = kswlib.make_params()
    pool, tasks = _tg().generate_seeds(p, n, "mixed100-300", seed=7200 + n)
    check(ctx, p, pool, tasks)
    check(ctx, p, pool, tasks)


def test_poisoned_seeds_among_good_ones(ctx):
    """seeds outside the range (device buffers only: the host-buffer call refuses them before it launches) get the failure
    record and raise BMH_E_RANGE; every other seed is exact, and so is the next call"""
    pkg = load_package()
    rng = np.random.default_rng(7300)
    p = kswlib.make_params()
    pool, tasks = _tg().generate_seeds(p, 2100, "mixed100-300", seed=7301)
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    bad = np.sort(rng.choice(len(tasks), 150, replace=False))
    broken = tasks.copy()
    for k, i in enumerate(bad):
        t = broken[i]
        if k % 5 == 0:
            t["len"] = 0
        elif k % 5 == 1:
            t["qbeg"] = -1
        elif k % 5 == 2:
            t["qbeg"] = t["l_query"] - t["len"] + 1  # the seed sticks out of the read
        elif k % 5 == 3:
            t["rbeg"] = -3
        else:
            t["wlen"] = t["rbeg"] + t["len"] - 1     # ... out of the window
        broken[i] = t
    good = np.ones(len(tasks), bool)
    good[bad] = False
    ctx.set_params(p)
    ctx.set_qcap(int(seed_flank(tasks).max()))
    for _ in range(2):
        s = dc.Seed(pool, broken)
        s.run(ctx)
        assert _sync_code(ctx) == pkg.BMH_E_RANGE
        got = s.result()
        dc.assert_seed(got[good], want[good], tasks[good], "beside poisoned seeds: ")
        assert (got[~good] == np.array([dc.SEED_FAIL], dtype=kswlib.SEED_RES)).all()
    s = dc.Seed(pool, tasks)
    s.run(ctx)
    ctx.sync()
    dc.assert_seed(s.result(), want, tasks, "after poisoned seeds: ")


@pytest.mark.parametrize("qcap", [40, 64, 100, 128])
def test_flanks_past_a_lowered_qcap(ctx, qcap):
    """a seed with a flank past qcap: failure record, BMH_E_RANGE, the others exact"""
    pkg = load_package()
    p = kswlib.make_params()
    pool, tasks = _tg().generate_seeds(p, 1500, "mixed100-300", seed=7400)
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    ok = seed_flank(tasks) <= qcap
    assert ok.any() and (~ok).any()
    ctx.set_params(p)
    ctx.set_qcap(qcap)
    for _ in range(2):
        s = dc.Seed(pool, tasks)
        s.run(ctx)
        assert _sync_code(ctx) == pkg.BMH_E_RANGE
        got = s.result()
        dc.assert_seed(got[ok], want[ok], tasks[ok], f"qcap {qcap}: ")
        assert (got[~ok] == np.array([dc.SEED_FAIL], dtype=kswlib.SEED_RES)).all()


def test_batch_above_the_fork_threshold(ctx):
    """more seeds than kForkMinTasks: the long bins run on the side stream"""
    p = kswlib.make_params()
    pool, tasks = _tg().generate_seeds(p, FORK_MIN_TASKS + 4321, "mixed100-300", seed=7500)
    check(ctx, p, pool, tasks)
    check(ctx, p, pool, tasks)


def test_flanks_on_both_sides_of_96_columns(ctx):
    """left and right flanks of 65..128 bases: the 65-128 bin's head of up to 96 columns is found through the sort's cursor at
    key 1023, which the make-and-bin pass has to leave as sort_hist_kernel did"""
    rng = np.random.default_rng(7600)
    p = kswlib.make_params()
    specs = []
    for _ in range(6000):
        lf, rf, ln = int(rng.integers(60, 133)), int(rng.integers(60, 133)), int(rng.integers(19, 32))
        specs.append((lf + ln + rf, lf, ln))
    pool, tasks = make_seeds(rng, specs)
    assert ((tasks["qbeg"] > 64) & (tasks["qbeg"] <= 96)).any() and ((tasks["qbeg"] > 96) & (tasks["qbeg"] <= 128)).any()
    check(ctx, p, pool, tasks)
    check(ctx, p, pool, tasks)


def test_wide_extension_bin(ctx):
    """the switch on, right flanks that start from a left score past 32000 (bin 6) among ordinary seeds"""
    rng = np.random.default_rng(7700)
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=300, w=100, pen_clip5=15, pen_clip3=15)
    a = wg.gen_seeds(rng, 14000, 6, qbegs=(11500, 12000, 12500, 13000))
    b = _tg().generate_seeds(p, 900, "mixed100-300", seed=7701)
    pool, tasks = concat_seeds(b, a)
    ctx.set_wide_extension(True)
    try:
        for _ in range(2):
            want, _ = check(ctx, p, pool, tasks)
            assert want["score"][-6:-2].min() > 32000
            ctx.seedext_batch(pool, tasks)
            assert ctx.extend_wide_stats()[0] >= 4
    finally:
        ctx.set_wide_extension(False)


def test_a_stale_hint_meets_another_batch(ctx):
    """calls in a row on one context whose left and right counts differ by orders of magnitude: the grids, the kernel of a bin
    and the (almost) empty round's single launch are chosen from the previous call's counts"""
    rng = np.random.default_rng(7800)
    p = kswlib.make_params()
    few_left = make_seeds(rng, [(int(L), 0 if k % 97 else 30, 25) for k, L in enumerate(rng.integers(80, 260, 4000))])
    few_right = make_seeds(rng, [(int(L), int(L) - 25 if k % 89 else 20, 25) for k, L in enumerate(rng.integers(80, 260, 4000))])
    many = _tg().generate_seeds(p, 30000, "mixed100-300", seed=7801)
    small = _tg().generate_seeds(p, 300, "150bp", seed=7802)
    for name, (pool, tasks) in (("few left", few_left), ("few left", few_left), ("many", many), ("few right", few_right),
                                ("few right", few_right), ("many", many), ("small", small), ("small", small), ("many", many),
                                ("few left", few_left)):
        check(ctx, p, pool, tasks, name + ": ")
