"""The lane-per-task global kernels on the band each task's result needs (host/glbband_core.h) against the oracle at the
tasks' own w: generator batches, one hand-made wave with every corner of the rule side by side, and a sparse permuted d_order (the
band travels with the position in the launch order, not with the task index).  Each batch also runs on a context created under
BMH_GLB_NARROW=0; the two outputs must be equal."""
import importlib

import numpy as np
import pytest

import devcalls as dc
import glbband_ref
import kswgen
import kswlib
from __graft_entry__ import load_package
from glbband_ref import w_eff  # the rule restated in Python
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu


def _tg():
    return importlib.import_module(load_package().__name__ + ".taskgen")


def _both(pool, tasks, words, p=None):
    """(results, CIGAR pool) of the default context, after checking that a context without the narrowing returns the same."""
    p = kswlib.make_params() if p is None else p
    out = []
    for env in ({}, {"BMH_GLB_NARROW": "0"}):
        ctx = _ctx_with(env)
        ctx.set_params(p)
        out.append(ctx.global_batch(pool, tasks, words))
        ctx.close()
    assert (out[0][0] == out[1][0]).all(), "narrowed and full-band results differ"
    for t, r in zip(tasks, out[0][0]):
        o, n = int(t["cigar_off"]), min(int(r["n_cigar"]), int(t["cigar_cap"]))
        assert np.array_equal(out[0][1][o:o + n], out[1][1][o:o + n]), "narrowed and full-band CIGARs differ"
    return out[0]


@pytest.mark.parametrize("workload,n", [("150bp", 4096), ("mixed100-300", 2048)])
def test_generator_tasks_match_the_oracle_at_their_own_band(workload, n):
    p = kswlib.make_params()
    pool, tasks, words = _tg().generate_global(n, workload, seed=939, wspread=32)
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    res, cig = _both(pool, tasks, words)
    dc.assert_glb(res, cig, want, wcig, tasks, workload + ": ")


def test_one_wave_with_every_corner_of_the_rule():
    """Fewer than 64 tasks, so that whichever lane kernel takes them they share waves: w_eff 0 beside w_eff 31, a task that moves from
    the 96-slot bin to the 64-slot one, w > 63 with w_eff <= 63, w == |delta|, w < |delta| on both sides (qlen > tlen + w: the
    reference's score is then -inf; tlen > qlen + w score only), score-only tasks, and tasks that stay in the wide bins."""
    rng = np.random.default_rng(4711)
    p = kswlib.make_params()
    pb, what = kswgen.PoolBuilder(kswlib.GLB_TASK), []
    base = kswgen.rand_seq(rng, 120)

    def sub(k, n=120):
        t = base[:n].copy()
        for x in rng.choice(n, size=k, replace=False):
            t[x] = (t[x] + 1) & 3
        return t

    def add(q, t, w, cigar=True):
        kswgen._add_glb(pb, q, t, w, cigar)
        what.append((w, w_eff(p, np.asarray(q), np.asarray(t), w), len(q), len(t), cigar))

    add(base, base.copy(), 20)                           # w_eff 0 ...
    add(base[:100], base[:69], 31)                       # ... beside w_eff 31 == |delta|
    add(base, sub(2), 40)                                # the 96-slot bin -> 64
    add(base, sub(1), 60)                                # the 128-slot bin -> 64
    add(base, sub(2), 100)                               # the wave kernel -> 64
    add(base, np.concatenate([base[:50], base[58:]]), 200)   # an 8-base deletion in the read's window, w > 63
    add(np.concatenate([base[:30], base[45:]]), base, 90)    # a 15-base insertion
    add(base[:110], base[:90], 20)                       # w == |delta|
    add(base[:90], base[:110], 20)
    add(base[:100], base[:80], 10)                       # w < |delta|: qlen > tlen + w
    add(base[:70], base[:45], 12)
    add(base[:80], base[:100], 10, cigar=False)          # ... and tlen > qlen + w (score only: the reference's traceback then starts outside
                                                         # the band, on direction bytes no row wrote)
    add(base, kswgen.rand_seq(rng, 120), 45)             # unrelated: stays in the 96-slot bin
    add(base, kswgen.rand_seq(rng, 115), 62)             # ... in the 128-slot bin
    add(base, kswgen.rand_seq(rng, 120), 80)             # ... with the wave kernel
    add(base, sub(3), 25)                                # the strictness case: w_eff 1
    add(base[:1], base[:1], 5)
    add(base[:1], base[:30], 40)
    for k in (0, 2, 5, 9, 14):                           # score only
        add(base, sub(k), 30 + 9 * k, cigar=False)
    for _ in range(20):                                  # ordinary neighbours for the same waves
        q = kswgen.rand_seq(rng, int(rng.integers(60, 151)))
        t = kswgen.mutate(rng, q, 0.03, 0.004, 0.004, 6)
        add(q, t if len(t) else q, abs(len(q) - len(t)) + int(rng.integers(0, 40)), rng.random() < 0.8)
    pool, tasks, words = kswgen.finish_glb(pb)
    assert len(tasks) < 64
    we = [x[1] for x in what]
    assert we[0] == 0 and we[1] == 31 and we[15] == 1
    assert 32 <= what[2][0] <= 47 and we[2] <= 31 and 48 <= what[3][0] <= 63 and we[3] <= 31
    assert all(w > 63 and e <= 63 for w, e, *_ in what[4:7]) and we[7] == 20 and we[8] == 20 and we[9] == 10 and we[10] == 12 and we[11] == 10
    assert 32 <= we[12] <= 47 and 48 <= we[13] <= 63 and we[14] > 63
    assert sum(not x[4] for x in what) >= 5
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=4)
    assert (want["score"][9:12] < -(1 << 29)).all()  # the reference's -inf
    res, cig = _both(pool, tasks, words)
    dc.assert_glb(res, cig, want, wcig, tasks, "corners: ")


def test_the_band_travels_with_the_position_in_a_sparse_order():
    """bmh_global_batch_device with a permuted d_order of 3 000 entries over 10 000 records: the results, and the bands the device
    computed (bmh_last_global_bands), entry k of which belongs to tasks[order[k]]."""
    rng = np.random.default_rng(4712)
    p = kswlib.make_params()
    pool, tasks, words = _tg().generate_global(10000, "150bp", seed=940, wspread=32)
    assert len(tasks) == 10000
    order = rng.permutation(len(tasks))[:3000].astype(np.uint32)
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    ctx = _ctx_with({})
    ctx.set_params(p)
    ctx.set_qcap(int(tasks["qlen"].max()))
    g = dc.Glb(pool, tasks, words, order)
    g.n = len(order)  # the launch covers the order's entries; the buffers hold all 10 000 records
    g.run(ctx)
    ctx.sync()
    bands = ctx.last_global_bands(len(order))  # the device's bands, by position in the order
    with pytest.raises(load_package().BmhError):
        ctx.last_global_bands(len(tasks))  # (the launch had 3 000 tasks, not 10 000)
    g.n = len(tasks)
    res, cig = g.result()
    ctx.close()
    rows_cap = min(int(tasks["qlen"].max()) + 2 * int(p["w"]) + 64, glbband_ref.ROWS_CAP)  # of a device-resident launch: from the capacity hint
    expect = glbband_ref.expected_bands(p, pool, tasks[order], rows_cap)
    bad = np.nonzero(bands != expect)[0]
    assert len(bad) == 0, f"{len(bad)} bands differ from the rule; first at position {bad[0]}: device={bands[bad[0]]} rule={expect[bad[0]]}"
    assert (expect != glbband_ref.expected_bands(p, pool, tasks[:len(order)], rows_cap)).sum() > 1000  # by task index it would be another list
    dc.assert_glb(res[order], cig, want[order], wcig, tasks[order], "sparse order: ")
    rest = np.setdiff1d(np.arange(len(tasks)), order)
    assert (res[rest].view(np.uint8) == res[rest].view(np.uint8)[0]).all(), "a record outside the order was written"
