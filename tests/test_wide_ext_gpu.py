"""The int32 extension kernel (extend_wide.hip) behind bmh_ctx_set_wide_extension, bit for bit against the oracle
(test_wide_ext_cpu.py pins the oracle to the reference there): flat batches on both sides of every switch of the dispatcher's
bin 6, the device entry point, the fused per-seed record, a sharded call and toggling the switch on one context.
bmh_extend_wide_stats shows, against widegen's copy of the dispatcher's condition, that the wide kernel really ran."""
import numpy as np
import pytest

import domaingen as dg
import kswlib
import widegen as wg
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with
from test_score_domain_gpu import EXT_GAPS_MSG, SEED_FIELDS, _seeds_at

pytestmark = pytest.mark.gpu


def _wide_ctx(env=None):
    ctx = _ctx_with(env or {})
    ctx.set_wide_extension(True)
    return ctx


def _cmp(ctx, p, pool, tasks, what):
    ctx.set_params(p)
    got = ctx.extend_batch(pool, tasks)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ; first task {tasks[bad[0]]} gpu={got[bad[0]]} oracle={want[bad[0]]}"
    n, _ = ctx.extend_wide_stats()
    assert n == wg.wide_count(p, tasks), f"{what}: the wide kernel received {n} tasks"
    return got


def _cmp_seed(ctx, p, pool, tasks, what):
    ctx.set_params(p)
    got = ctx.seedext_batch(pool, tasks)
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    for f in SEED_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}, {f}: {len(bad)} differ; first seed {tasks[bad[0]]} gpu={got[bad[0]]} oracle={want[bad[0]]}"
    return got


def test_wide_flat_batches_on_both_sides_of_every_switch():
    rng = np.random.default_rng(8100)
    on, off = _wide_ctx(), _ctx_with({})
    # a mixed batch: in-range tasks give exactly what the default context gives them, the others go wide
    for p in (kswlib.make_params(a=10, b=40, o_del=60, e_del=10, o_ins=60, e_ins=10, zdrop=1000), kswlib.make_params(a=3)):
        pool, tasks = wg.gen_mixed(rng, p)
        wide = np.array([wg.goes_wide(p, int(t["qlen"]), int(t["h0"])) for t in tasks])
        assert 0 < wide.sum() < len(tasks)
        got = _cmp(on, p, pool, tasks, "mixed")
        off.set_params(p)
        assert (off.extend_batch(pool, tasks[~wide]) == got[~wide]).all()
        assert got["score"][wide].max() > 32000
    # just above 32000, and scores of millions
    p = kswlib.make_params(a=5, b=20, o_del=30, e_del=3, o_ins=30, e_ins=3, zdrop=2000)
    specs = [(100, 31501), (100, 31502), (6201, 1000), (6202, 1000), (300, 3_000_000), (2000, 5_000_000), (9000, 16_000_000 - 45_000)]
    pool, tasks = wg.gen_ext(rng, p, specs)
    sums = np.maximum(tasks["h0"], 0) + tasks["qlen"].astype(np.int64) * 5
    assert {32001, 32005, 32010} <= set(sums.tolist()) and sums.max() > 15_000_000
    assert (_cmp(on, p, pool, tasks, "score range")["score"][4:] > 3_000_000).all()
    # the LDS kernel's query cap +-1 (a = 1: in range up to 13 632 columns), in one batch whose longest query is past it
    p = kswlib.make_params(a=1, b=4, zdrop=200)
    pool, tasks = wg.gen_ext(rng, p, [(wg.LDS_QCAP - 1, 100), (wg.LDS_QCAP, 100), (wg.LDS_QCAP + 1, 100), (500, 100)])
    assert [wg.goes_wide(p, int(t["qlen"]), 100) for t in tasks] == [False, False, True, False]
    _cmp(on, p, pool, tasks, "LDS kernel cap")
    # the wide kernel's LDS/HBM cutoff +-1 (a = 3: all three are wide); the variant is chosen per task inside a batch
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=600)
    for qs in ((wg.WIDE_LDS_QCAP - 1, wg.WIDE_LDS_QCAP), (wg.WIDE_LDS_QCAP - 1, wg.WIDE_LDS_QCAP, wg.WIDE_LDS_QCAP + 1)):
        pool, tasks = wg.gen_ext(rng, p, [(q, 100) for q in qs])
        _cmp(on, p, pool, tasks, f"wide LDS/HBM cutoff {qs}")
    # the widest query the task record holds, with a modest band
    p = kswlib.make_params(a=1, b=4)
    pool, tasks = wg.gen_ext(rng, p, [(65535, 100), (40000, 1000), (14000, 30000)], w=(20,), indel=0.0)
    assert tasks["qlen"].max() == 65535
    assert (_cmp(on, p, pool, tasks, "qlen 65535")["qle"] > 10000).all()
    # gap costs past 16 bits: the whole batch goes wide
    for g in wg.WIDE_GAP_SETS:
        p = kswlib.make_params(a=2, b=4, zdrop=100, **g)
        assert not dg.ext_gaps_accepted(p)
        pool, tasks = wg.gen_ext(rng, p, [(q, h) for q in (30, 200, 700) for h in (0, 50, 3000)], w=(5, 50), indel=0.02)
        _cmp(on, p, pool, tasks, f"gaps {g}")
    on.close(), off.close()


def test_wide_mode_switch_sends_every_task_to_the_wide_kernel():
    """BMH_EXT_MODE=wide on a context with the switch on: in-range tasks on the int32 kernel give what the 16-bit kernels give."""
    rng = np.random.default_rng(8150)
    ctx = _wide_ctx({"BMH_EXT_MODE": "wide", "BMH_EXT_SMALL": "0"})
    p = kswlib.make_params(a=1, b=4)
    pool, tasks = wg.gen_mixed(rng, p, n_in=200, n_wide=0)
    ctx.set_params(p)
    ctx.set_kernel_timing(True)
    got = ctx.extend_batch(pool, tasks)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    assert (got == want).all()
    n, ms = ctx.extend_wide_stats()
    assert n == len(tasks) and ms > 0
    ctx.close()


def test_wide_device_entry_with_qcap():
    import torch
    pkg = load_package()
    rng = np.random.default_rng(8200)
    ctx = _wide_ctx()
    dev = torch.device("cuda:0")
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=600)
    ctx.set_params(p)

    def run(pool, tasks):
        d_pool = torch.from_numpy(pool).to(dev)
        d_tasks = torch.from_numpy(tasks.view(np.uint8)).to(dev)
        d_res = torch.zeros(len(tasks) * kswlib.EXT_RES.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.extend_batch_device(d_pool.data_ptr(), d_tasks.data_ptr(), len(tasks), d_res.data_ptr())
        ctx.sync()
        return d_res.cpu().numpy().view(kswlib.EXT_RES)

    pool, tasks = wg.gen_ext(rng, p, [(100, 50), (400, 31000), (12000, 100), (20000, 100), (15000, 100)])
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    ctx.set_qcap(12000)  # the 20 000 / 15 000 column tasks are refused on the device ...
    with pytest.raises(pkg.BmhError) as e:
        run(pool, tasks)
    assert e.value.code == pkg.BMH_E_RANGE
    ctx.set_qcap(20000)  # ... and served once the capacity covers them (HBM slab)
    got = run(pool, tasks)
    assert (got == want).all()
    assert ctx.extend_wide_stats()[0] == wg.wide_count(p, tasks) == 4
    ctx.close()


def test_wide_fused_seed_record():
    rng = np.random.default_rng(8300)
    ctx = _wide_ctx()
    # -A 3 on reads of 10 667 bp and more: l_query*a past 32000 (refused by default)
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=300, w=100, pen_clip5=15, pen_clip3=15)
    pool, seeds = _seeds_at(rng, 10667, 6)
    _cmp_seed(ctx, p, pool, seeds, "-A 3, 10 667 bp")  # (refused by the seed bound; each flank still fits 16 bits)
    # right flanks that start from a left score past 32000 (h0 of the right task)
    pool, seeds = wg.gen_seeds(rng, 14000, 8, qbegs=(11500, 12000, 12500, 13000))
    got = _cmp_seed(ctx, p, pool, seeds, "-A 3, 14 kb")
    assert got["score"][:4].min() > 32000
    assert ctx.extend_wide_stats()[0] >= 4  # at least those four right flanks ran on the wide kernel
    # narrow bands and indels force both retries (left and right at 2w)
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=300, w=4, pen_clip5=15, pen_clip3=15)
    pool, seeds = wg.gen_seeds(rng, 11000, 24, indel=0.003)
    _cmp_seed(ctx, p, pool, seeds, "narrow bands")
    st = ctx.seedext_stats()
    assert st["left_retries"] > 0 and st["right_retries"] > 0
    ctx.close()


def test_wide_sharded_on_two_contexts():
    pkg = load_package()
    rng = np.random.default_rng(8400)
    ctxs = [_wide_ctx(), _wide_ctx()]
    p = kswlib.make_params(a=10, b=40, o_del=60, e_del=10, o_ins=60, e_ins=10, zdrop=1000)
    for c in ctxs:
        c.set_params(p)
    pool, tasks = wg.gen_mixed(rng, p, n_in=40, n_wide=16)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    assert (pkg.extend_batch_sharded(ctxs, pool, tasks) == want).all()
    assert sum(c.extend_wide_stats()[0] for c in ctxs) == wg.wide_count(p, tasks)
    spool, seeds = _seeds_at(rng, 4000, 16)  # -A 10 on 4 kb reads
    got = pkg.seedext_batch_sharded(ctxs, spool, seeds)
    swant, _, _ = kswlib.orc_seedext_batch(p, spool, seeds, nthreads=8)
    for f in SEED_FIELDS:
        assert (got[f] == swant[f]).all(), f
    for c in ctxs:
        c.close()


def test_wide_toggle_restores_the_exact_refusals():
    pkg = load_package()
    rng = np.random.default_rng(8500)
    ctx = _wide_ctx()

    def refused(fn, msg):
        with pytest.raises(pkg.BmhError) as e:
            fn()
        assert e.value.code == pkg.BMH_E_RANGE and msg in str(e.value), str(e.value)

    p = kswlib.make_params(a=5, b=20, o_del=30, e_del=3, o_ins=30, e_ins=3)
    pool, tasks = wg.gen_ext(rng, p, [(100, 31501), (6401, 0), (300, 100)])
    spool, seeds = _seeds_at(rng, 6401, 3)
    gp = kswlib.make_params(o_del=0, e_del=16384, o_ins=0, e_ins=16384)
    gpool, gtasks = wg.gen_ext(rng, gp, [(150, 0), (150, 20)])
    _cmp(ctx, p, pool, tasks, "on")
    _cmp_seed(ctx, p, spool, seeds, "seeds on")
    _cmp(ctx, gp, gpool, gtasks, "gaps on")
    ctx.set_wide_extension(False)
    ctx.set_params(p)
    refused(lambda: ctx.extend_batch(pool, tasks), "h0 + qlen*max(mat) exceeds the 16-bit score range")
    refused(lambda: ctx.seedext_batch(spool, seeds), "l_query*max(max(mat), a) exceeds the 16-bit score range")
    ctx.set_params(gp)
    refused(lambda: ctx.extend_batch(gpool, gtasks), EXT_GAPS_MSG)
    assert ctx.extend_wide_stats() == (0, -1.0)
    pool, tasks = wg.gen_mixed(rng, p, n_wide=0)
    ctx.set_params(p)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    assert (ctx.extend_batch(pool, tasks) == want).all()
    ctx.close()
