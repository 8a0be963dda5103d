"""A context carries state from call to call: the bin-size hints per call kind (bmh_ctx::BinHint: "a stale or missing hint costs
speed, never correctness"), the tiny-list path they select for device-counted lists, bin 3's choice between the two-lanes-per-task
and the one-wave-per-task kernel, grow-only workspaces that still hold earlier contents, the error flag, and the gap-cost
instantiation picked per call.  Each test drives one fresh context through an explicit call sequence -- host-buffer calls
wait at exit, so the next call sees the previous call's hint -- and checks every result against the oracle."""
import importlib

import numpy as np
import pytest

import devcalls as dc
import domaingen as dg
import kswgen
import kswlib
import widegen as wg
from __graft_entry__ import load_package
from test_device_entry_gpu import concat_ext, seed_flank
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

LANEX_MIN_TASKS = 4096  # kLanexMinTasks, extend_dispatch.hip
TINY_LIST = 2048        # kTinyList, extend_dispatch.hip
ASYM = dict(o_del=6, e_del=1, o_ins=4, e_ins=2)


def _tg():
    load_package()
    return importlib.import_module("bwa_mem_quickassist_amd.taskgen")


def _ext_cmp(ctx, p, pool, tasks, what=""):
    ctx.set_params(p)
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    dc.assert_ext(ctx.extend_batch(pool, tasks), want, tasks, what)


def _seed_cmp(ctx, p, pool, tasks, what=""):
    ctx.set_params(p)
    want, _, calls = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    dc.assert_seed(ctx.seedext_batch(pool, tasks), want, tasks, what)
    st = ctx.seedext_stats()
    assert st["seeds"] == len(tasks)
    assert st["left_tasks"] + st["left_retries"] + st["right_tasks"] + st["right_retries"] == calls, what
    return st


def _bin3_flanks(rng, n):
    """n extension tasks of 129-256 query columns (bin 3 of the lane-per-task dispatcher)."""
    pool, tasks = wg.gen_ext(rng, None, [(int(rng.integers(129, 257)), int(rng.integers(20, 120))) for _ in range(n)])
    assert all(dg.ext_bin(int(q)) == 3 for q in tasks["qlen"])
    return pool, tasks


@pytest.mark.parametrize("gaps", ["symmetric", "asymmetric"])
def test_bin3_kernel_choice_follows_the_hint(gaps):
    """5 000, 300, 9 000, 300 flanks of 129-256 columns: no hint (both kernels look at the count), a hint of 5 000 (lanes per
    task), a hint of 300 (one wave per task on a grid sized for ~1 000: it has to stride over 9 000), a hint of 9 000."""
    rng = np.random.default_rng(9700)
    p = kswlib.make_params(**(ASYM if gaps == "asymmetric" else {}))
    ctx = _ctx_with({"BMH_EXT_SMALL": "0"})  # (small batches would go to the one-task-per-wave kernels in every bin)
    big, small, bigger = _bin3_flanks(rng, 5000), _bin3_flanks(rng, 300), _bin3_flanks(rng, 9000)
    assert len(big[1]) >= LANEX_MIN_TASKS > len(small[1]) and len(bigger[1]) > 8 * 1024
    for k, (pool, tasks) in enumerate([big, small, bigger, small]):
        _ext_cmp(ctx, p, pool, tasks, f"{gaps}, call {k}: ")
    ctx.close()


def test_tiny_retry_path_outgrown():
    """A fused call with few retries leaves hints of <= 2 048 for the retry rounds (kinds 2 and 4); the next call, 60 000 seeds at w = 8,
    starts its retry rounds on the tiny path (one LDS launch over the device-counted list) with lists far longer than that; a
    large default-band call then starts from the tiny path's bin-5-only hint."""
    tg = _tg()
    ctx = _ctx_with({})
    p = kswlib.make_params(w=100)
    pool, tasks = tg.generate_seeds(p, 3000, "150bp", seed=9710)
    st = _seed_cmp(ctx, p, pool, tasks, "few retries: ")
    assert st["left_retries"] <= TINY_LIST and st["right_retries"] <= TINY_LIST, st
    p8 = kswlib.make_params(w=8)
    pool, tasks = tg.generate_seeds(p8, 60000, "mixed100-300", seed=9711)
    st = _seed_cmp(ctx, p8, pool, tasks, "w = 8 on the tiny path: ")
    assert st["left_retries"] > TINY_LIST and st["right_retries"] > TINY_LIST, st
    pool, tasks = tg.generate_seeds(p, 30000, "mixed100-300", seed=9712)
    _seed_cmp(ctx, p, pool, tasks, "default band after the tiny path: ")
    # and the device form on the same context, its lists counted on the device only
    ctx.set_qcap(int(seed_flank(tasks).max()))
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    for pp in (p8, p):
        ctx.set_params(pp)
        s = dc.Seed(pool, tasks)
        s.run(ctx)
        ctx.sync()
        if pp is p:
            dc.assert_seed(s.result(), want, tasks, "device form: ")
    ctx.close()


@pytest.mark.parametrize("env", [{}, {"BMH_EXT_PERSIST": "1", "BMH_EXT_SMALL": "0"}, {"BMH_EXT_SPLIT96": "0", "BMH_EXT_SMALL": "0"}],
                         ids=["auto", "persist", "nosplit96"])
def test_hints_across_parameter_switches(env):
    """One context, one call after the other: symmetric and asymmetric gaps, a general matrix, zdrop -1 / 0 / 100, the wide
    extension on, off and on again -- each call runs with the hints of the one before, under other parameters."""
    rng = np.random.default_rng(9720)
    tg = _tg()
    ctx = _ctx_with(env)
    gen = kswlib.make_params(mat=dg.big_matrix(rng, a=6, lo=-8))
    sets = [("default", kswlib.make_params()), ("asymmetric", kswlib.make_params(**ASYM)), ("general matrix", gen),
            ("symmetric again", kswlib.make_params(w=40)), ("zdrop -1", kswlib.make_params(zdrop=-1)),
            ("zdrop 0", kswlib.make_params(zdrop=0)), ("zdrop 100, asymmetric", kswlib.make_params(zdrop=100, **ASYM))]
    epool, etasks, _ = tg.generate(kswlib.make_params(), 12000, "mixed100-300", seed=9721)
    spool, seeds = tg.generate_seeds(kswlib.make_params(), 4000, "mixed100-300", seed=9722)
    for k, (name, p) in enumerate(sets):
        n = [len(etasks), 700, 5000][k % 3]  # batch sizes change too
        _ext_cmp(ctx, p, epool, etasks[:n], f"{name}, extension: ")
        _seed_cmp(ctx, p, spool, seeds[: [4000, 300][k % 2]], f"{name}, fused: ")
    p = kswlib.make_params(a=3, b=9, o_del=18, e_del=3, o_ins=18, e_ins=3, zdrop=600)
    wpool, wtasks = concat_ext((epool, etasks[:3000]), wg.gen_mixed(rng, p, n_in=16, n_wide=8))
    wide = wg.wide_count(p, wtasks)
    assert wide > 0
    inside = np.array([not wg.goes_wide(p, int(t["qlen"]), int(t["h0"])) for t in wtasks])
    for on in (True, False, True):
        ctx.set_wide_extension(on)
        if on:
            _ext_cmp(ctx, p, wpool, wtasks, "wide on: ")
            assert ctx.extend_wide_stats()[0] == wide
        else:
            _ext_cmp(ctx, p, wpool, wtasks[inside], "wide off: ")
            with pytest.raises(load_package().BmhError):
                ctx.extend_batch(wpool, wtasks)
    ctx.close()


def test_shrinking_after_growth():
    """A large batch grows every workspace; the small calls of other kinds after it run over what it left behind."""
    tg = _tg()
    rng = np.random.default_rng(9730)
    p = kswlib.make_params()
    ctx = _ctx_with({})
    pool, tasks, _ = tg.generate(p, 40000, "mixed100-300", seed=9731)
    _ext_cmp(ctx, p, pool, tasks, "large: ")
    spool, seeds = tg.generate_seeds(p, 60, "250bp", seed=9732)
    _seed_cmp(ctx, p, spool, seeds, "small fused after large: ")
    gpool, gtasks, gwords = tg.generate_global(40, "150bp", seed=9733)
    gwant, gwcig, _ = kswlib.orc_global_batch_mt(p, gpool, gtasks, gwords, nthreads=8)
    dc.assert_glb(*ctx.global_batch(gpool, gtasks, gwords), gwant, gwcig, gtasks, "small global after large: ")
    wpool, wtasks = tg.generate_sw(p, 40, "150bp", seed=9734)
    wwant, _ = kswlib.orc_sw_batch(p, wpool, wtasks, nthreads=8)
    dc.assert_sw(ctx.sw_batch(wpool, wtasks), wwant, wtasks, "small sw after large: ")
    _ext_cmp(ctx, p, pool, tasks[:7], "7 tasks after large: ")
    e = dc.Ext(pool, tasks[:50])
    ctx.set_qcap(int(tasks["qlen"].max()))
    e.run(ctx)
    ctx.sync()
    want, _ = kswlib.orc_extend_batch(p, pool, tasks[:50], nthreads=8)
    dc.assert_ext(e.result(), want, tasks[:50], "device, 50 after large: ")
    ctx.close()
    # reserved ahead, then given more than was reserved
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.reserve_device(4096, 100, 256)
    ctx.reserve_kernels(100, 150, 100, 150)
    _ext_cmp(ctx, p, pool, tasks[:5000], "past reserve_device: ")
    gpool, gtasks, gwords = tg.generate_global(3000, "mixed100-300", seed=9735)
    gwant, gwcig, _ = kswlib.orc_global_batch_mt(p, gpool, gtasks, gwords, nthreads=8)
    dc.assert_glb(*ctx.global_batch(gpool, gtasks, gwords), gwant, gwcig, gtasks, "past reserve_kernels: ")
    _seed_cmp(ctx, p, spool, seeds, "fused after reserve: ")
    ctx.close()


def test_seeded_random_call_sequence():
    """About 40 calls of every kind, host and device forms, random sizes and two parameter sets, on one context."""
    seed = 9740
    rng = np.random.default_rng(seed)
    tg = _tg()
    params = [kswlib.make_params(), kswlib.make_params(w=30, zdrop=50, **ASYM)]
    epool, etasks, _ = tg.generate(params[0], 30000, "mixed100-300", seed=9741)
    spool, seeds = tg.generate_seeds(params[0], 8000, "mixed100-300", seed=9742)
    gpool, gtasks, gwords = tg.generate_global(4000, "mixed100-300", seed=9743)
    wpool, wtasks = tg.generate_sw(params[0], 4000, "150bp", seed=9744)
    want = []
    for p in params:
        want.append(dict(ext=kswlib.orc_extend_batch(p, epool, etasks, nthreads=8)[0],
                         seed=kswlib.orc_seedext_batch(p, spool, seeds, nthreads=8)[0],
                         glb=kswlib.orc_global_batch_mt(p, gpool, gtasks, gwords, nthreads=8)[:2],
                         sw=kswlib.orc_sw_batch(p, wpool, wtasks, nthreads=8)[0]))
    ctx = _ctx_with({})
    ctx.set_qcap(max(int(etasks["qlen"].max()), int(seed_flank(seeds).max()), int(gtasks["qlen"].max())))
    for call in range(40):
        kind = str(rng.choice(["ext", "seed", "glb", "sw"]))
        form = str(rng.choice(["host", "device"]))
        pk = int(rng.integers(0, 2))
        p, W = params[pk], want[pk]
        total = {"ext": len(etasks), "seed": len(seeds), "glb": len(gtasks), "sw": len(wtasks)}[kind]
        n = int(rng.choice([1, 17, 300, 2500, total]))
        lo = int(rng.integers(0, total - n + 1))
        sel = slice(lo, lo + n)
        what = f"seed {seed}, call {call}: {kind} {form} n={n} params {pk}: "
        ctx.set_params(p)
        if kind == "ext":
            got = ctx.extend_batch(epool, etasks[sel]) if form == "host" else _dev(ctx, dc.Ext(epool, etasks[sel]))
            dc.assert_ext(got, W["ext"][sel], etasks[sel], what)
        elif kind == "seed":
            got = ctx.seedext_batch(spool, seeds[sel]) if form == "host" else _dev(ctx, dc.Seed(spool, seeds[sel]))
            dc.assert_seed(got, W["seed"][sel], seeds[sel], what)
        elif kind == "glb":
            res, cig = ctx.global_batch(gpool, gtasks[sel], gwords) if form == "host" else _dev(ctx, dc.Glb(gpool, gtasks[sel], gwords))
            dc.assert_glb(res, cig, W["glb"][0][sel], W["glb"][1], gtasks[sel], what)
        else:
            got = ctx.sw_batch(wpool, wtasks[sel]) if form == "host" else _dev(ctx, dc.Sw(wpool, wtasks[sel]))
            dc.assert_sw(got, W["sw"][sel], wtasks[sel], what)
    ctx.close()


def _dev(ctx, job):
    job.run(ctx)
    ctx.sync()
    return job.result()
