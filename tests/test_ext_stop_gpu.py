"""The extension lane kernels end a flank once no later row can change its result (host/extstop_core.h).  Every batch
runs on a context with the rule and on one created under BMH_EXT_STOP=0: the results must be the oracle's both times, and with the
rule on the rows each task ran (bmh_last_extend_rows) must be those of the rule restated in Python (tests/extstop_ref.py), task by
task -- equal results alone would also pass a rule that never fires."""
import numpy as np
import pytest

import devcalls as dc
import extstop_cases as xc
import extstop_ref
import kswgen
import kswlib
from test_device_entry_gpu import _tg, seed_flank
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

LANE = {"BMH_EXT_SMALL": "0"}  # (small batches would go to the one-task-per-wave kernels, which run every row)
NO_LANE = 0xffff
EDGES = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
SCORINGS = {"default": dict(), "asym": dict(o_del=6, e_del=1, o_ins=4, e_ins=2), "zdrop5": dict(zdrop=5),
            "A<0": dict(mat=np.minimum(kswlib.fill_scmat(1, 4), -1))}  # the last: max(mat) < 0, the rule does not apply


def _edges(rng, per=40):
    """qlen on both sides of every instantiation's width, tlen = 2 qlen + 8."""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for L in EDGES:
        for k in range(per):
            q, t = kswgen.flank_pair(rng, L, L + 8, 0.02 + 0.1 * (k % 4 == 3), 0.004, 0.004, 3)
            kswgen._add_ext(pb, rng, q, t, int(rng.integers(19, 130)) if k % 5 else int(rng.integers(0, 19)), 100, 5)
    return pb.finish()


def _one_key(rng, L=60, n=75):
    """Tasks of one query length, h0 bucket and target length -- one sort key, so they share waves -- that stop at very different rows:
    at once (unrelated), a few rows behind the diagonal (perfect), at the last row (the query's end never reached)."""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for k in range(n):
        q = kswgen.rand_seq(rng, L)
        tail = kswgen.rand_seq(rng, L + 8)
        t = [np.concatenate([q, tail]), kswgen.rand_seq(rng, 2 * L + 8), np.concatenate([q[:L // 2], tail, tail]),
             np.concatenate([q[:L - 9], kswgen.rand_seq(rng, 4), q[L - 9:], tail])][k % 4][:2 * L + 8]
        kswgen._add_ext(pb, rng, q, t, 40 + k % 8, 3 if k % 8 == 7 else 100, 5)
    return pb.finish()


@pytest.fixture(scope="module")
def batches():
    """{name: (pool, tasks)}; `all`: the edges, the targeted cases in every instantiation, one-key waves and the tiny tasks."""
    rng = np.random.default_rng(8100)
    targeted = xc.merge([xc.targeted(rng, L, reps=1)[:2] for L in (20, 32, 33, 50, 64, 65, 80, 96, 97, 110, 128)])
    b = {"targeted": targeted, "edges": _edges(rng), "one_key": _one_key(rng), "tiny": xc.tiny(rng)}
    b["all"] = xc.merge([b["edges"], b["targeted"], b["one_key"], b["tiny"]])
    q = b["all"][1]["qlen"]
    assert len(q) <= 4096 and all(((q > lo) & (q <= hi)).sum() % 64 for lo, hi in ((0, 32), (32, 64), (64, 96), (96, 128)))  # every bin ends in a partial wave
    return b


_want = {}


def want(batches, name, scoring):
    """(params, oracle results, rows with the rule) of a batch under a scoring, computed once."""
    key = (name, scoring)
    if key not in _want:
        p = kswlib.make_params(**SCORINGS[scoring])
        pool, tasks = batches[name]
        orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
        rows, out = extstop_ref.rows(p, pool, tasks)
        assert (out == orc).all(), "the Python restatement's outputs differ from the oracle's"
        _want[key] = (p, orc, rows)
    return _want[key]


def run(env, p, pool, tasks):
    """(results, rows) of bmh_extend_batch on a fresh context"""
    ctx = _ctx_with({**LANE, **env})
    try:
        ctx.set_params(p)
        ctx.set_extend_rows(len(tasks))
        got = ctx.extend_batch(pool, tasks)
        return got, ctx.last_extend_rows(len(tasks)).astype(np.int64)
    finally:
        ctx.close()


def assert_rows(rows, want_rows, tasks, what=""):
    lane = tasks["qlen"] <= 128
    assert (rows[~lane] == NO_LANE).all()
    bad = np.nonzero(lane & (rows != want_rows))[0]
    assert len(bad) == 0, f"{what}rows differ for {len(bad)} of {int(lane.sum())} tasks; first {bad[0]}: gpu {rows[bad[0]]} want {want_rows[bad[0]]} task {tasks[bad[0]]}"


@pytest.mark.parametrize("env", [{}, {"BMH_EXT_PERSIST": "1"}, {"BMH_EXT_SPLIT96": "0"}], ids=["grid", "persist", "no96"])
def test_rows_and_results_default_scoring(batches, env):
    pool, tasks = batches["all"]
    p, orc, rows = want(batches, "all", "default")
    got, grows = run(env, p, pool, tasks)
    print(f"{len(tasks)} tasks, rows per task: rule {grows.mean():.1f}, restated {rows.mean():.1f}")
    dc.assert_ext(got, orc, tasks, "rule on: ")
    assert_rows(grows, rows, tasks)
    for L in EDGES:  # the rule fires in every instantiation: most flanks of 2 qlen + 8 rows end well before their last row
        sel = (tasks["qlen"] == L) & (tasks["tlen"] == 2 * L + 8)
        assert sel.sum() >= 40 and grows[sel].mean() < 1.5 * L + 8, (L, grows[sel].mean())  # (the reference: 2 L + 8 for a good flank)


def test_switch_off_runs_the_references_rows(batches):
    pool, tasks = batches["all"]
    p, orc, rows = want(batches, "all", "default")
    got, grows = run({"BMH_EXT_STOP": "0"}, p, pool, tasks)
    dc.assert_ext(got, orc, tasks, "rule off: ")
    assert (grows >= rows).all() and (grows > rows).mean() > 0.5
    full, _ = extstop_ref.rows(p, *batches["one_key"], rule=False)
    off = len(batches["edges"][1]) + len(batches["targeted"][1])
    assert_rows(grows[off:off + len(full)], full, batches["one_key"][1], "rule off: ")


@pytest.mark.parametrize("scoring", ["asym", "zdrop5", "A<0"])
def test_other_scorings(batches, scoring):
    """a non-default scoring the rule applies to, a small z-drop (breaking before, at and after the rule's row), and a matrix
    without a non-negative entry, for which the rule does not apply: the rows are then the reference's"""
    pool, tasks = batches["targeted"]
    p, orc, rows = want(batches, "targeted", scoring)
    for env in ({}, {"BMH_EXT_STOP": "0"}):
        got, grows = run(env, p, pool, tasks)
        dc.assert_ext(got, orc, tasks, f"{scoring} {env}: ")
        if not env:
            assert_rows(grows, rows, tasks, scoring + ": ")
    if scoring == "A<0":
        assert not extstop_ref.rule_applies(p)
        assert_rows(grows, rows, tasks, "A<0, rule off: ")  # (rows: the reference's, since the rule does not apply)
    elif scoring == "asym":
        assert (grows > rows).any()


def test_sparse_order(batches):
    """bmh_extend_batch_device over every third task in a shuffled order: rows by task index, 0xffff for the tasks not listed"""
    pool, tasks = batches["all"]
    p, orc, rows = want(batches, "all", "default")
    rng = np.random.default_rng(8200)
    order = rng.permutation(np.arange(0, len(tasks), 3)).astype(np.uint32)
    ctx = _ctx_with(LANE)
    try:
        ctx.set_params(p)
        ctx.set_qcap(128)
        ctx.set_extend_rows(len(tasks))
        e = dc.Ext(pool, tasks, order)
        # (not e.run: that passes len(tasks) for n, and n is the number of entries of d_order)
        ctx.extend_batch_device(e.pool.data_ptr(), e.tasks.data_ptr(), len(order), e.res.data_ptr(), e.order.data_ptr())
        ctx.sync()
        got, grows = e.result(), ctx.last_extend_rows(len(tasks)).astype(np.int64)
    finally:
        ctx.close()
    listed = np.zeros(len(tasks), bool)
    listed[order] = True
    dc.assert_ext(got[listed], orc[listed], tasks[listed], "sparse order: ")
    assert (got[~listed].view(np.uint8) == dc.POISON).all() and (grows[~listed] == NO_LANE).all()
    assert_rows(grows[listed], rows[listed], tasks[listed], "sparse order: ")


def test_stale_hint_sends_the_96_column_head_to_the_128_column_launch(batches):
    """the second launch's 65-128 bin is sized from the first one's handful of tasks, so the head launch reaches only the back of
    the 65-96 column tasks and the 128-column launch takes the rest of them (`rem` in the kernel)"""
    rng = np.random.default_rng(8300)
    few = xc.merge([xc.targeted(rng, 80, reps=1)[:2], batches["tiny"]])
    parts = [kswgen.PoolBuilder(kswlib.EXT_TASK)]
    for k in range(900):
        L = int(rng.integers(65, 97)) if k % 4 else int(rng.integers(97, 129))
        q, t = kswgen.flank_pair(rng, L, L + 8)
        kswgen._add_ext(parts[0], rng, q, t, int(rng.integers(19, 100)), 100, 5)
    pool, tasks = parts[0].finish()
    assert (tasks["qlen"] <= 96).sum() > len(few[1]) + 64 + 128
    p = kswlib.make_params()
    orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    rows, _ = extstop_ref.rows(p, pool, tasks)
    ctx = _ctx_with(LANE)
    try:
        ctx.set_params(p)
        for _ in range(2):
            ctx.extend_batch(*few)  # (the call waits for its results: the bin counts have landed before the next launch polls them)
        ctx.set_extend_rows(len(tasks))
        got = ctx.extend_batch(pool, tasks)
        grows = ctx.last_extend_rows(len(tasks)).astype(np.int64)
    finally:
        ctx.close()
    dc.assert_ext(got, orc, tasks, "stale hint: ")
    assert_rows(grows, rows, tasks, "stale hint: ")


def test_rows_are_off_by_default_and_bounded_by_the_cap(batches):
    pool, tasks = batches["tiny"]
    ctx = _ctx_with(LANE)
    try:
        ctx.extend_batch(pool, tasks)
        with pytest.raises(Exception):
            ctx.last_extend_rows(len(tasks))  # nothing was recorded
        ctx.set_extend_rows(10)  # fewer entries than tasks: the first ten are recorded, nothing is written behind them
        got = ctx.extend_batch(pool, tasks)
        assert (ctx.last_extend_rows(10) != NO_LANE).all()
        with pytest.raises(Exception):
            ctx.last_extend_rows(11)
        orc, _ = kswlib.orc_extend_batch(kswlib.make_params(), pool, tasks)
        dc.assert_ext(got, orc, tasks)
    finally:
        ctx.close()


def test_fused_seed_call_matches_the_oracle():
    p = kswlib.make_params()
    pool, tasks = _tg().generate_seeds(p, 2048, "150bp", seed=8400)
    tasks = tasks[:2048]
    want_, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    for env in ({}, {"BMH_EXT_STOP": "0"}):
        ctx = _ctx_with({**LANE, **env})
        try:
            ctx.set_qcap(max(int(seed_flank(tasks).max()), 1))
            s = dc.Seed(pool, tasks)
            s.run(ctx)
            ctx.sync()
            dc.assert_seed(s.result(), want_, tasks, f"{env}: ")
        finally:
            ctx.close()
