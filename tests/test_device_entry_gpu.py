"""The *_device entry points (what bench.py times) against the oracle: the qcap contract of bmh_ctx_set_qcap, launch orders
(d_order), the caller's stream (bmh_ctx_set_stream) with the extension bins forked onto side streams, two contexts on two
caller streams, and the two-step fused per-seed call (bmh_seedext_submit / _wait) over a resident pool (bmh_upload_pool).
Every device result buffer is filled with a poison byte before the call (devcalls.py)."""
import numpy as np
import pytest

import devcalls as dc
import globallong as gl
import kswgen
import kswlib
import widegen as wg
from __graft_entry__ import load_package
from test_global_long_gpu import _ordinary
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

FORK_MIN_TASKS = 131072  # kForkMinTasks, bwa-mem-quickassist_amd/csrc/extend_dispatch.hip


def _tg():
    import importlib
    load_package()
    return importlib.import_module("bwa_mem_quickassist_amd.taskgen")


def _sync_code(ctx):
    """ctx.sync() -> 0 or the error code it raised."""
    pkg = load_package()
    try:
        ctx.sync()
    except pkg.BmhError as e:
        return e.code
    return 0


def concat_ext(*batches):
    pools, tasks, off = [], [], 0
    for pool, t in batches:
        t = t.copy()
        t["q_off"] += off
        t["t_off"] += off
        pools.append(pool), tasks.append(t)
        off += len(pool)
    return np.concatenate(pools), np.concatenate(tasks)


def concat_seeds(*batches):
    return concat_ext(*batches)  # (the same two offsets)


def seed_flank(tasks):
    """The longer flank of every seed: the query length of its left or right extension."""
    return np.maximum(tasks["qbeg"], tasks["l_query"] - tasks["qbeg"] - tasks["len"])


def long_seeds(rng, lens, slen=30, ctxlen=40):
    """One seed per read length in `lens`: a random read, its window (the read with 1 % substitutions between `ctxlen` random
    bases on either side) and a `slen`-base exact seed at a random place -- flanks up to the read length."""
    pb = kswgen.PoolBuilder(kswlib.SEED_TASK)
    for L in lens:
        read = kswgen.rand_seq(rng, L)
        mid = kswgen.mutate(rng, read, 0.01, 0.0, 0.0)
        qbeg = int(rng.integers(0, L - slen + 1))
        mid[qbeg:qbeg + slen] = read[qbeg:qbeg + slen]
        win = np.concatenate([kswgen.rand_seq(rng, ctxlen), mid, kswgen.rand_seq(rng, ctxlen)])
        qo, to = pb.put(read), pb.put(win)
        pb.tasks.append((qo, to, L, qbeg, slen, ctxlen + qbeg, len(win), 0, 0))
    return pb.finish()


# ---- the qcap contract --------------------------------------------------------------------------------------------------

QCAPS = [32, 64, 100, 128, 200, 256, 300, 512]
EXT_QLENS = [1, 16, 32, 33, 48, 64, 65, 100, 101, 128, 129, 200, 201, 256, 257, 300, 301, 320, 512, 513, 700, 1500]


@pytest.fixture(scope="module")
def qcap_ext():
    rng = np.random.default_rng(9100)
    p = kswlib.make_params()
    pool, tasks = wg.gen_ext(rng, p, [(q, int(rng.integers(20, 120))) for q in EXT_QLENS for _ in range(3)])
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    return p, pool, tasks, want


@pytest.mark.parametrize("env", [{}, {"BMH_EXT_SMALL": "0"}], ids=["auto", "lane"])
def test_extend_device_qcap_contract(qcap_ext, env):
    """Tasks up to qcap are exact, longer ones carry the failure record, sync() reports BMH_E_RANGE, and the next call on the
    same context is clean -- for caps inside every bin and at its edges."""
    pkg = load_package()
    p, pool, tasks, want = qcap_ext
    ctx = _ctx_with(env)
    ctx.set_params(p)
    for qcap in QCAPS:
        ctx.set_qcap(qcap)
        e = dc.Ext(pool, tasks)
        e.run(ctx)
        code = _sync_code(ctx)
        got = e.result()
        ok = tasks["qlen"] <= qcap
        dc.assert_ext(got[ok], want[ok], tasks[ok], f"qcap {qcap}: ")
        over = got[~ok]
        fail = np.array([dc.EXT_FAIL], dtype=kswlib.EXT_RES)
        bad = np.nonzero(over != fail)[0]
        assert len(bad) == 0, (f"qcap {qcap}: {len(bad)} of {len(over)} tasks over the cap lack the failure record; first: "
                               f"qlen {tasks[~ok][bad[0]]['qlen']} -> {over[bad[0]]}")
        assert code == pkg.BMH_E_RANGE, f"qcap {qcap}: sync() returned {code} with {len(over)} tasks over the cap"
        # the next call on the same context: every task inside the cap, no error left behind
        ctx.set_qcap(int(tasks["qlen"].max()))
        e = dc.Ext(pool, tasks)
        e.run(ctx)
        ctx.sync()
        dc.assert_ext(e.result(), want, tasks, f"after qcap {qcap}: ")
    ctx.close()


@pytest.fixture(scope="module")
def qcap_seeds():
    rng = np.random.default_rng(9200)
    p = kswlib.make_params()
    a = _tg().generate_seeds(p, 600, "mixed100-300", seed=9201)
    b = long_seeds(rng, [400, 400, 700, 700, 1100, 1100, 1100])
    pool, tasks = concat_seeds(a, b)
    want, _, _ = kswlib.orc_seedext_batch(p, pool, tasks, nthreads=8)
    return p, pool, tasks, want


def test_seedext_device_qcap_contract(qcap_seeds):
    """A seed with a flank longer than qcap gets the record of a seed outside the range (score = truesc = INT32_MIN, other
    fields 0) and sync() reports BMH_E_RANGE; the other seeds are exact."""
    pkg = load_package()
    p, pool, tasks, want = qcap_seeds
    ctx = _ctx_with({})
    ctx.set_params(p)
    flank = seed_flank(tasks)
    for qcap in QCAPS:
        ctx.set_qcap(qcap)
        s = dc.Seed(pool, tasks)
        s.run(ctx)
        code = _sync_code(ctx)
        got = s.result()
        ok = flank <= qcap
        dc.assert_seed(got[ok], want[ok], tasks[ok], f"qcap {qcap}: ")
        over = got[~ok]
        bad = np.nonzero(over != np.array([dc.SEED_FAIL], dtype=kswlib.SEED_RES))[0]
        assert len(bad) == 0, f"qcap {qcap}: {len(bad)} of {len(over)} seeds over the cap: first {tasks[~ok][bad[0]]} -> {over[bad[0]]}"
        assert code == (pkg.BMH_E_RANGE if (~ok).any() else 0), f"qcap {qcap}: sync() returned {code}, {(~ok).sum()} seeds over the cap"
        ctx.set_qcap(int(flank.max()))
        s = dc.Seed(pool, tasks)
        s.run(ctx)
        ctx.sync()
        dc.assert_seed(s.result(), want, tasks, f"after qcap {qcap}: ")
    ctx.close()


def test_host_buffer_entries_ignore_qcap(qcap_ext, qcap_seeds):
    """The host-buffer entry points size their launches from the tasks: a small qcap must not touch them."""
    ctx = _ctx_with({})
    p, pool, tasks, want = qcap_ext
    ctx.set_params(p)
    ctx.set_qcap(32)
    dc.assert_ext(ctx.extend_batch(pool, tasks), want, tasks)
    p, pool, tasks, want = qcap_seeds
    ctx.set_params(p)
    dc.assert_seed(ctx.seedext_batch(pool, tasks), want, tasks)
    ctx.close()


# ---- launch orders ------------------------------------------------------------------------------------------------------

def _orders(rng, qlen):
    return {"permuted": rng.permutation(len(qlen)).astype(np.uint32),
            "by_length": np.argsort(-qlen.astype(np.int64), kind="stable").astype(np.uint32)}


@pytest.mark.parametrize("env,wide", [({}, False), ({"BMH_EXT_SMALL": "0"}, False), ({"BMH_EXT_MODE": "lanex4"}, False),
                                      ({"BMH_EXT_SMALL": "0"}, True)], ids=["auto", "lane", "lanex4", "lane-wide"])
def test_extend_device_order(env, wide):
    """d_order: results stay at task index, for tasks in every bin (and bin 6 with the wide extension on)."""
    rng = np.random.default_rng(9300)
    p = kswlib.make_params()
    specs = [(int(rng.integers(lo, hi + 1)), int(rng.integers(20, 150)))
             for lo, hi in [(1, 32), (33, 64), (65, 96), (97, 128), (129, 256), (257, 512), (513, 1200)] for _ in range(40)]
    batch = wg.gen_ext(rng, p, specs)
    if wide:
        batch = concat_ext(batch, wg.gen_mixed(rng, p, n_in=16, n_wide=8))
    pool, tasks = batch
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    ctx = _ctx_with(env)
    ctx.set_params(p)
    ctx.set_wide_extension(wide)
    ctx.set_qcap(int(tasks["qlen"].max()))
    for name, order in _orders(rng, tasks["qlen"]).items():
        for _ in range(2):  # the second call runs with the first one's bin-size hints
            e = dc.Ext(pool, tasks, order)
            e.run(ctx)
            ctx.sync()
            dc.assert_ext(e.result(), want, tasks, f"{name}: ")
    if wide:
        assert ctx.extend_wide_stats()[0] == wg.wide_count(p, tasks) > 0
    ctx.close()


def test_global_device_order():
    """d_order on the global path: every lane bin, the wave kernel and one band-ring task; results and CIGAR words at task index."""
    rng = np.random.default_rng(9400)
    p = kswlib.make_params()
    pool, tasks, words = gl.concat(_ordinary(rng), gl.gen_long(rng, [(12000, 50, "cigar")]))
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    routes = set(gl.route(p, tasks, long_bin=True).tolist())
    assert {0, 1, 2, 3, 4} <= routes, routes
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.set_qcap(int(tasks["qlen"].max()))
    for name, order in _orders(rng, tasks["qlen"]).items():
        g = dc.Glb(pool, tasks, words, order)
        g.run(ctx)
        ctx.sync()
        res, cig = g.result()
        dc.assert_glb(res, cig, want, wcig, tasks, f"{name}: ")
    assert ctx.global_long_stats()[0] == 2
    ctx.close()


# ---- the caller's stream ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_ext():
    """>= kForkMinTasks extension tasks (mixed 100-300 bp flanks, every bin): 40 k generated tasks, tiled over one pool."""
    p = kswlib.make_params()
    pool, base, _ = _tg().generate(p, 20000, "mixed100-300", seed=9500)
    reps = -(-FORK_MIN_TASKS // len(base)) + 1
    want, _ = kswlib.orc_extend_batch(p, pool, base, nthreads=8)
    return p, pool, np.tile(base, reps), np.tile(want, reps)


@pytest.fixture(scope="module")
def others():
    """A fused per-seed batch, a global batch and a mate-rescue batch, with their oracle results."""
    tg = _tg()
    p = kswlib.make_params()
    spool, seeds = tg.generate_seeds(p, 4000, "mixed100-300", seed=9501)
    swant, _, _ = kswlib.orc_seedext_batch(p, spool, seeds, nthreads=8)
    gpool, gtasks, gwords = tg.generate_global(3000, "150bp", seed=9502)
    gwant, gwcig, _ = kswlib.orc_global_batch_mt(p, gpool, gtasks, gwords, nthreads=8)
    wpool, wtasks = tg.generate_sw(p, 3000, "150bp", seed=9503)
    wwant, _ = kswlib.orc_sw_batch(p, wpool, wtasks, nthreads=8)
    return dict(p=p, seed=(spool, seeds, swant), glb=(gpool, gtasks, gwords, gwant, gwcig), sw=(wpool, wtasks, wwant))


@pytest.mark.parametrize("sched", [None, 0, 1, 2, 3, 4])
def test_extend_device_on_callers_stream(big_ext, sched):
    """set_stream: the whole launch, the side streams' bins included, is ordered behind the caller's stream -- waiting on that
    stream alone is enough.  Then set_stream(0) gives the context its own stream back."""
    import torch
    p, pool, tasks, want = big_ext
    assert len(tasks) >= FORK_MIN_TASKS
    ctx = _ctx_with({} if sched is None else {"BMH_EXT_SCHED": str(sched)})
    ctx.set_params(p)
    ctx.set_qcap(int(tasks["qlen"].max()))
    s = torch.cuda.Stream(dc.dev())
    ctx.set_stream(s.cuda_stream)
    e = dc.Ext(pool, tasks)
    e.run(ctx)
    s.synchronize()
    dc.assert_ext(e.result(), want, tasks, f"sched {sched}, caller's stream: ")
    ctx.set_stream(0)
    e = dc.Ext(pool, tasks)
    e.run(ctx)
    ctx.sync()
    dc.assert_ext(e.result(), want, tasks, f"sched {sched}, own stream: ")
    ctx.close()


def test_other_device_entries_on_callers_stream(others):
    import torch
    p = others["p"]
    spool, seeds, swant = others["seed"]
    gpool, gtasks, gwords, gwant, gwcig = others["glb"]
    wpool, wtasks, wwant = others["sw"]
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.set_qcap(max(int(seed_flank(seeds).max()), int(gtasks["qlen"].max())))
    s = torch.cuda.Stream(dc.dev())
    ctx.set_stream(s.cuda_stream)
    sd, g, w = dc.Seed(spool, seeds), dc.Glb(gpool, gtasks, gwords), dc.Sw(wpool, wtasks)
    sd.run(ctx)
    g.run(ctx)
    w.run(ctx)
    s.synchronize()
    dc.assert_seed(sd.result(), swant, seeds, "caller's stream: ")
    dc.assert_glb(*g.result(), gwant, gwcig, gtasks, "caller's stream: ")
    dc.assert_sw(w.result(), wwant, wtasks, "caller's stream: ")
    ctx.set_stream(0)
    sd, g, w = dc.Seed(spool, seeds), dc.Glb(gpool, gtasks, gwords), dc.Sw(wpool, wtasks)
    sd.run(ctx)
    g.run(ctx)
    w.run(ctx)
    ctx.sync()
    dc.assert_seed(sd.result(), swant, seeds, "own stream: ")
    dc.assert_glb(*g.result(), gwant, gwcig, gtasks, "own stream: ")
    dc.assert_sw(w.result(), wwant, wtasks, "own stream: ")
    ctx.close()


def test_two_contexts_two_callers_streams(big_ext, others):
    """As bench.py's extension contexts: both enqueued before either is waited for."""
    import torch
    p, pool, tasks, want = big_ext
    spool, seeds, swant = others["seed"]
    ctxs = [_ctx_with({}) for _ in range(2)]
    streams = [torch.cuda.Stream(dc.dev()) for _ in ctxs]
    for c, s in zip(ctxs, streams):
        c.set_params(p)
        c.set_qcap(max(int(tasks["qlen"].max()), int(seed_flank(seeds).max())))
        c.set_stream(s.cuda_stream)
    e, sd = dc.Ext(pool, tasks), dc.Seed(spool, seeds)
    sd2 = dc.Seed(spool, seeds[::-1].copy())
    e.run(ctxs[0])
    sd.run(ctxs[1])
    sd2.run(ctxs[0])
    for s in streams:
        s.synchronize()
    dc.assert_ext(e.result(), want, tasks, "context 0: ")
    dc.assert_seed(sd.result(), swant, seeds, "context 1: ")
    dc.assert_seed(sd2.result(), swant[::-1], seeds[::-1], "context 0, second call: ")
    for c in ctxs:
        c.set_stream(0)
        c.sync()
        c.close()


# ---- two-step fused per-seed call, resident pool ------------------------------------------------------------------------

def test_seedext_submit_wait(others):
    pkg = load_package()
    p = others["p"]
    spool, seeds, swant = others["seed"]
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.upload_pool(spool)
    ctx.seedext_submit(seeds)
    host = kswlib.orc_seedext_batch(p, spool, seeds[:200], nthreads=1)[0]  # host work while the device runs
    got = ctx.seedext_wait()
    st = ctx.seedext_stats()
    dc.assert_seed(got, swant, seeds, "submit/wait: ")
    assert (host == swant[:200]).all()
    ref = ctx.seedext_batch(spool, seeds)
    assert (ref == got).all()
    assert ctx.seedext_stats() == st and st["seeds"] == len(seeds)
    # the host-buffer form against the resident pool
    assert (ctx.seedext_batch(None, seeds) == swant).all()
    # an empty submission
    ctx.seedext_submit(seeds[:0])
    assert len(ctx.seedext_wait()) == 0
    # refusals, each leaving the context usable
    for what in ("twice", "nothing pending"):
        with pytest.raises(pkg.BmhError) as e:
            if what == "twice":
                ctx.seedext_submit(seeds[:100])
                try:
                    ctx.seedext_submit(seeds[:50])
                finally:
                    got = ctx.seedext_wait()  # the first submission is still delivered
                    dc.assert_seed(got, swant[:100], seeds[:100], "after a refused second submission: ")
            else:
                ctx.seedext_wait()
        assert e.value.code == pkg.BMH_E_ARG, what
        dc.assert_seed(ctx.seedext_batch(spool, seeds[:300]), swant[:300], seeds[:300], f"after {what}: ")
    ctx.close()
    bare = _ctx_with({})  # no resident pool
    bare.set_params(p)
    with pytest.raises(pkg.BmhError) as e:
        bare.seedext_submit(seeds[:10])
    assert e.value.code == pkg.BMH_E_ARG
    dc.assert_seed(bare.seedext_batch(spool, seeds[:300]), swant[:300], seeds[:300], "after a submission without a pool: ")
    bare.close()


def test_extend_and_global_against_resident_pool():
    rng = np.random.default_rng(9600)
    p = kswlib.make_params()
    epool, etasks = kswgen.gen_ext_realistic(rng, 800, read_len=(100, 300))
    ewant, _ = kswlib.orc_extend_batch(p, epool, etasks, nthreads=8)
    gpool, gtasks, words = _ordinary(rng)
    gwant, gwcig, _ = kswlib.orc_global_batch_mt(p, gpool, gtasks, words, nthreads=8)
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.upload_pool(epool)
    dc.assert_ext(ctx.extend_batch(None, etasks), ewant, etasks, "resident pool: ")
    dc.assert_ext(ctx.extend_batch(None, etasks[::3]), ewant[::3], etasks[::3], "resident pool, again: ")
    ctx.upload_pool(gpool)  # replaces the first
    res, cig = ctx.global_batch(None, gtasks, words)
    dc.assert_glb(res, cig, gwant, gwcig, gtasks, "resident pool: ")
    ctx.close()
