"""The extension lane kernels run each flank on the band its six outputs need (host/extband_core.h).  Every batch's
results must be the oracle's at the task's OWN w, and the band the device computed per task (bmh_last_extend_bands) must be that of
the rule restated in Python (tests/extband_ref.py), by input position -- equal results alone would also pass a pass that never
narrows.  With BMH_EXT_NARROW=0, and with the rows diagnostic armed, every task runs on its own band."""
import numpy as np
import pytest

import devcalls as dc
import extband_cases as bc
import extband_ref
import extstop_cases as xc
import extstop_ref
import kswgen
import kswlib
from test_device_entry_gpu import _tg, seed_flank
from test_kernel_families_gpu import _ctx_with
from test_pac_resident_gpu import _pac_tasks

pytestmark = pytest.mark.gpu

LANE = {"BMH_EXT_SMALL": "0"}  # (small batches would go to the one-task-per-wave kernels, which keep the task's band)
QLENS = (1, 8, 9, 31, 32, 33, 64, 65, 96, 97, 128)
SCORINGS = {"default": dict(), "asym": dict(o_del=6, e_del=1, o_ins=4, e_ins=2), "zdrop12": dict(zdrop=12), "a3": dict(a=3, b=4, o_del=5, e_del=2, o_ins=5, e_ins=2),
            "A<0": dict(mat=np.minimum(kswlib.fill_scmat(1, 4), -1))}  # the last: max(mat) < 0, the rule leaves every task alone


def _edges(rng, per=44):
    """qlen on both sides of every instantiation's width: good flanks (most are narrowed), some with indels, a low h0 or a narrow w"""
    pb = kswgen.PoolBuilder(kswlib.EXT_TASK)
    for L in QLENS:
        for k in range(per):
            q, t = kswgen.flank_pair(rng, L, 8 + k % 9, 0.02 + 0.1 * (k % 4 == 3), 0.02 * (k % 6 == 5), 0.02 * (k % 6 == 5), 3)
            kswgen._add_ext(pb, rng, q, t, int(rng.integers(19, 130)) if k % 5 else int(rng.integers(0, 19)), (100, 100, 7, 2)[k % 4], 5)
    return pb.finish()


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(9100)
    targeted = xc.merge([xc.targeted(rng, L, reps=1)[:2] for L in (20, 33, 64, 80, 97, 128)])
    b = {"edges": _edges(rng), "handmade": bc.handmade(rng)[:2], "boundary": bc.boundary(rng)[:2], "targeted": targeted, "tiny": xc.tiny(rng)}
    b["all"] = xc.merge([b["edges"], b["handmade"], b["boundary"], b["targeted"], b["tiny"]])
    assert len(b["all"][1]) <= 4096
    return b


_want = {}


def want(batches, name, scoring):
    """(params, oracle results at the tasks' own w, expected band bytes) of a batch under a scoring, computed once"""
    key = (name, scoring)
    if key not in _want:
        p = kswlib.make_params(**SCORINGS[scoring])
        pool, tasks = batches[name]
        orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
        _want[key] = (p, orc, extband_ref.expected_bands(p, pool, tasks))
    return _want[key]


def run(env, p, pool, tasks, rows=False):
    """(results, bands[, rows]) of bmh_extend_batch on a fresh context"""
    ctx = _ctx_with({**LANE, **env})
    try:
        ctx.set_params(p)
        if rows:
            ctx.set_extend_rows(len(tasks))
        got = ctx.extend_batch(pool, tasks)
        bands = ctx.last_extend_bands(len(tasks))
        return (got, bands, ctx.last_extend_rows(len(tasks)).astype(np.int64)) if rows else (got, bands)
    finally:
        ctx.close()


def assert_bands(bands, want_bands, tasks, what=""):
    bad = np.nonzero(bands != want_bands)[0]
    assert len(bad) == 0, f"{what}bands differ for {len(bad)} of {len(tasks)} tasks; first {bad[0]}: gpu {bands[bad[0]]} want {want_bands[bad[0]]} task {tasks[bad[0]]}"


@pytest.mark.parametrize("env", [{}, {"BMH_EXT_PERSIST": "1"}, {"BMH_EXT_SPLIT96": "0"}, {"BMH_EXT_BANDKEY": "0"}], ids=["grid", "persist", "no96", "h0key"])
def test_results_and_bands_default_scoring(batches, env):
    pool, tasks = batches["all"]
    p, orc, wb = want(batches, "all", "default")
    got, bands = run(env, p, pool, tasks)
    narrowed = wb < np.minimum(tasks["w"], 255)
    print(f"{len(tasks)} tasks, {narrowed.sum()} narrowed, mean band of those {wb[narrowed].mean():.2f}")
    dc.assert_ext(got, orc, tasks, "narrowing on: ")
    assert_bands(bands, wb, tasks)
    for L in QLENS[1:]:  # the rule bites in every instantiation (qlen 1: the clamped band is 1 anyway)
        sel = (tasks["qlen"] == L) & (tasks["w"] == 100)
        assert sel.sum() >= 20 and narrowed[sel].mean() > 0.3, (L, narrowed[sel].mean())


def test_switch_off_lists_every_tasks_own_band(batches):
    pool, tasks = batches["all"]
    p, orc, wb = want(batches, "all", "default")
    got, bands = run({"BMH_EXT_NARROW": "0"}, p, pool, tasks)
    dc.assert_ext(got, orc, tasks, "narrowing off: ")
    assert_bands(bands, extband_ref.expected_bands(p, pool, tasks, narrow=False), tasks, "narrowing off: ")
    assert (bands == np.minimum(tasks["w"], 255)).all()


def test_rows_diagnostic_runs_the_full_band(batches):
    """armed, bmh_last_extend_rows reports the rows of the reference's band: those of tests/extstop_ref.py, which knows no narrowing"""
    pool, tasks = xc.merge([batches["edges"], batches["boundary"]])
    p = kswlib.make_params()
    orc, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    rows, out = extstop_ref.rows(p, pool, tasks)
    assert (out == orc).all()
    got, bands, grows = run({}, p, pool, tasks, rows=True)
    dc.assert_ext(got, orc, tasks, "rows armed: ")
    assert (bands == np.minimum(tasks["w"], 255)).all()
    lane = tasks["qlen"] <= 128
    assert (grows[lane] == rows[lane]).all()


@pytest.mark.parametrize("scoring", ["asym", "zdrop12", "a3", "A<0"])
def test_other_scorings(batches, scoring):
    pool, tasks = xc.merge([batches["targeted"], batches["boundary"], batches["handmade"]])
    key = ("tbh", scoring)
    if key not in _want:
        p = kswlib.make_params(**SCORINGS[scoring])
        _want[key] = (p, kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)[0], extband_ref.expected_bands(p, pool, tasks))
    p, orc, wb = _want[key]
    got, bands = run({}, p, pool, tasks)
    dc.assert_ext(got, orc, tasks, scoring + ": ")
    assert_bands(bands, wb, tasks, scoring + ": ")
    narrowed = (wb < np.minimum(tasks["w"], 255)).sum()
    assert (narrowed == 0) if scoring == "A<0" else (narrowed > 10), (scoring, narrowed)


def test_sparse_order(batches):
    """bmh_extend_batch_device over every third task in a shuffled order: band k belongs to tasks[order[k]]"""
    pool, tasks = batches["all"]
    p, orc, wb = want(batches, "all", "default")
    rng = np.random.default_rng(9200)
    order = rng.permutation(np.arange(0, len(tasks), 3)).astype(np.uint32)
    ctx = _ctx_with(LANE)
    try:
        ctx.set_params(p)
        ctx.set_qcap(128)
        e = dc.Ext(pool, tasks, order)
        ctx.extend_batch_device(e.pool.data_ptr(), e.tasks.data_ptr(), len(order), e.res.data_ptr(), e.order.data_ptr())
        ctx.sync()
        got, bands = e.result(), ctx.last_extend_bands(len(order))
        with pytest.raises(Exception):
            ctx.last_extend_bands(len(tasks))  # (the launch had len(order) entries)
    finally:
        ctx.close()
    listed = np.zeros(len(tasks), bool)
    listed[order] = True
    dc.assert_ext(got[listed], orc[listed], tasks[listed], "sparse order: ")
    assert (got[~listed].view(np.uint8) == dc.POISON).all()
    assert_bands(bands, wb[order], tasks[order], "sparse order: ")


def test_small_batches_have_no_band_pass(batches):
    pool, tasks = batches["tiny"]
    ctx = _ctx_with({})  # (below the small-batch threshold: one task per wave, the task's own band)
    try:
        got = ctx.extend_batch(pool, tasks)
        with pytest.raises(Exception):
            ctx.last_extend_bands(len(tasks))
        orc, _ = kswlib.orc_extend_batch(kswlib.make_params(), pool, tasks)
        dc.assert_ext(got, orc, tasks)
    finally:
        ctx.close()


def test_packed_and_reversed_targets():
    """BMH_F_TPAC targets (both strands of the 2-bit reference) and reversed flanks: the bands of the same flanks addressed by bytes"""
    rng = np.random.default_rng(9300)
    l_pac = 100003
    pac, pool, tp, tb = _pac_tasks(rng, 700, l_pac, (60, 140))
    p = kswlib.make_params()
    wb = extband_ref.expected_bands(p, pool, tb)
    want_p, _ = kswlib.orc_extend_batch(p, pool, tp, nthreads=4, pac=pac, l_pac=l_pac)
    assert (wb < np.minimum(tb["w"], 255)).mean() > 0.3
    ctx = _ctx_with(LANE)
    try:
        ctx.set_pac(pac, l_pac)
        for tasks in (tp, tb):
            got = ctx.extend_batch(pool, tasks)
            bands = ctx.last_extend_bands(len(tasks))
            dc.assert_ext(got, want_p, tasks, "packed: " if tasks is tp else "bytes: ")
            assert_bands(bands, wb, tasks)
    finally:
        ctx.close()


@pytest.mark.parametrize("w", [100, 3])
def test_fused_seed_call_matches_the_oracle(w):
    """w = 3: max_off >= 3w/4 sends many flanks of both sides through the retry rounds, which run un-narrowed at 2w"""
    p = kswlib.make_params(w=w)
    pool, tasks = _tg().generate_seeds(p, 2048, "mixed100-300" if w == 3 else "150bp", seed=9400)
    tasks = tasks[:2048]
    want_, _, calls = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    has = (tasks["qbeg"] > 0).astype(int) + (tasks["qbeg"] + tasks["len"] != tasks["l_query"]).astype(int)
    retried = want_["n_ext"] - has
    print(f"w {w}: {len(tasks)} seeds, {calls} extensions, {int((retried > 0).sum())} seeds retried, {int((retried == 2).sum())} on both sides")
    if w == 3:
        assert (retried == 2).any() and (retried == 1).any()
    for env in ({}, {"BMH_EXT_NARROW": "0"}):
        ctx = _ctx_with({**LANE, **env})
        try:
            ctx.set_params(p)
            ctx.set_qcap(max(int(seed_flank(tasks).max()), 1))
            s = dc.Seed(pool, tasks)
            s.run(ctx)
            ctx.sync()
            dc.assert_seed(s.result(), want_, tasks, f"{env}: ")
        finally:
            ctx.close()
