"""The band the device computes per task (glb_band_kernel, read back with bmh_last_global_bands) against the rule restated in Python
(glbband_ref.py), byte for byte and by input position, and the results on those bands against the oracle at the tasks' own w: score,
n_cigar and every CIGAR word.  Every assertion is an equality.

The rule's bound is loose by design (every remaining pair is taken to score max(mat)), so a device band a few diagonals too narrow
rarely changes a result and one too wide never does: equal results do not show that the band is the rule's.  The read-back does.

  1. every (q, t) over two letters up to length 5 and over three letters up to length 3, at every w, under six scorings;
  2. narrowing onto each side of the bin limits 15/16, 31/32, 47/48, 63/64;
  3. the optimal path on the outermost diagonal of the band, on either side, at d = 15, 31, 47, 63 (the last slot of the 32-, 64-, 96-
     and 128-slot kernels) and around them;
  4. the eight-lane split of the band pass as the device executes it: the best gap position on, before and after every part boundary;
  5. (in test_global_band_gpu.py) by position and not by task index, with a sparse permuted d_order.

Each batch runs on a default context, with BMH_GLB_C32=0 (bands up to 15 on the 64-slot kernel) and with BMH_GL_FAST=0, and its
results are compared with a context under BMH_GLB_NARROW=0.

The scoring 'e0' has no gap extension cost: bmh_ctx_set_params takes such parameters for the global calls alone."""
import numpy as np
import pytest

import devcalls as dc
import glbband_ref as gr
import kswgen
import kswlib
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

ENVS = ({}, {"BMH_GLB_C32": "0"}, {"BMH_GL_FAST": "0"})
LIMITS = ((15, 16), (31, 32), (47, 48), (63, 64))


def _check(p, batch, envs=ENVS, what=""):
    """Runs the batch under every environment: results == the oracle's at w, bands == the restatement's; then the same results
    without the narrowing, where there is no band to read.  Returns the bands."""
    pool, tasks, words = batch
    n = len(tasks)
    assert not (tasks["tlen"].astype(np.int64) > tasks["qlen"].astype(np.int64) + tasks["w"]).any()  # (the reference's traceback is undefined there)
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    expect = gr.expected_bands(p, pool, tasks)
    first = None
    for env in envs + ({"BMH_GLB_NARROW": "0"},):
        ctx = _ctx_with(env)
        try:
            ctx.set_params(p)
            res, cig = ctx.global_batch(pool, tasks, words)
            dc.assert_glb(res, cig, want, wcig, tasks, f"{what}{env}: ")
            if "BMH_GLB_NARROW" in env:
                with pytest.raises(load_package().BmhError) as e:
                    ctx.last_global_bands(n)
                assert e.value.code == load_package().BMH_E_ARG
                assert (res == first).all(), "narrowed and full-band results differ"
                continue
            bands = ctx.last_global_bands(n)
            bad = np.nonzero(bands != expect)[0]
            assert len(bad) == 0, (f"{what}{env}: {len(bad)} of {n} device bands differ from the rule; first at position {bad[0]}: "
                                   f"task={tasks[bad[0]]} device={bands[bad[0]]} rule={expect[bad[0]]}")
            first = res if first is None else first
        finally:
            ctx.close()
    return expect


# ---- 1. exhaustive small shapes ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_sets():
    a, b = gr.set_a(), gr.set_b()
    assert len(a[1]) == 22732 and len(b[1]) == 6741 and (a[1]["cigar_cap"] > 0).all() and (b[1]["cigar_cap"] > 0).all()
    return a, b


@pytest.mark.parametrize("scoring", list(gr.SCORINGS))
def test_every_small_pair_at_every_band(small_sets, scoring):
    """Sets A (22 732 tasks) and B (6 741), all of them in the 32-slot kernel and with BMH_GLB_C32=0 in the 64-slot one.
    e0 has no gap extension cost: such parameters serve the global calls alone (bmh_ctx_set_params)."""
    p = kswlib.make_params(**gr.SCORINGS[scoring])
    for name, batch in zip("AB", small_sets):
        expect = _check(p, batch, what=f"{scoring}/{name}: ")
        assert (expect <= 15).all()  # the 32-slot kernel's; with BMH_GLB_C32=0 the 64-slot one's
        if name == "A":
            assert 7000 < int((expect < batch[1]["w"]).sum()) < 18000  # narrowed, and not all of them


# ---- 2. narrowing onto each side of every bin limit -------------------------------------------------------------------------------

def _subst(rng, s, k):
    t = s.copy()
    for x in rng.choice(len(s), size=k, replace=False):
        t[x] = (t[x] + 1 + rng.integers(0, 3)) & 3
    return t


def _equal_len_band(p, k, L=150, w=100):
    """The rule's band for equal lengths L and k substitutions: it depends on k alone (the restatement, on one such pair)."""
    q = np.zeros(L, dtype=np.uint8)
    t = q.copy()
    t[:k] = 1
    return gr.w_eff(p, q, t, w)


@pytest.mark.parametrize("scoring", ["default", "asymmetric"])
def test_narrowing_onto_each_side_of_every_bin_limit(scoring):
    rng = np.random.default_rng(5150)
    p = kswlib.make_params(**gr.SCORINGS[scoring])
    L, w = 150, 100
    ks = [3, 11, 12, 21, 22, 30, 31, 32, 40, 41]
    if scoring == "default":  # floor((5k - 12) / 3)
        assert [_equal_len_band(p, k) for k in ks] == [1, 14, 16, 31, 32, 46, 47, 49, 62, 64]
        assert all(_equal_len_band(p, k) == (5 * k - 12) // 3 for k in range(3, 60))
    by_k = {k: _equal_len_band(p, k) for k in range(0, 90)}
    for lo, hi in LIMITS:  # the nearest k on either side of every limit that the rule reaches under this scoring
        ks.append(max(k for k, e in by_k.items() if e <= lo))
        ks.append(min(k for k, e in by_k.items() if e >= hi))
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for k in sorted(set(ks)):
        for _ in range(2):
            q = kswgen.rand_seq(rng, L)
            t = _subst(rng, q, k)
            x = int(rng.integers(10, L - 10))
            ins = kswgen.rand_seq(rng, 5)
            kswgen._add_glb(pb, q, t, w)                                           # delta 0
            kswgen._add_glb(pb, np.concatenate([q[:x], ins, q[x:]]), t, w)         # one 5-base insertion: delta +5
            kswgen._add_glb(pb, q, np.concatenate([t[:x], ins, t[x:]]), w)         # one 5-base deletion: delta -5
    batch = kswgen.finish_glb(pb)
    bands = _check(p, batch, what=f"{scoring}: ")
    eq = bands[0::3]
    assert sorted(set(eq)) == sorted({by_k[k] for k in ks})
    for lo, hi in LIMITS:
        assert (eq <= lo).any() and (eq >= hi).any() and max(eq[eq <= lo]) >= lo - 2 and min(eq[eq >= hi]) <= hi + 2
    for lo, hi in ((0, 15), (16, 31), (32, 47), (48, 63), (64, 255)):  # no instantiation is skipped without notice
        for part in (bands[0::3], bands[1::3], bands[2::3]):
            assert int(((part >= lo) & (part <= hi)).sum()) >= 2, (scoring, lo, hi)


# ---- 3. the optimum on the outermost diagonal -------------------------------------------------------------------------------------

DIAGS = (1, 2, 7, 8, 14, 15, 16, 30, 31, 32, 46, 47, 48, 62, 63, 64)


@pytest.mark.parametrize("scoring", ["default", "asymmetric", "scaled", "open0"])
def test_optimum_on_the_outermost_diagonal(scoring):
    rng = np.random.default_rng(6300)
    p = kswlib.make_params(**gr.SCORINGS[scoring])
    pb, pw = kswgen.PoolBuilder(kswlib.GLB_TASK), kswgen.PoolBuilder(kswlib.GLB_TASK)
    for d in DIAGS:
        for ls in (120, 200):
            s, x, y = kswgen.rand_seq(rng, ls), kswgen.rand_seq(rng, d), kswgen.rand_seq(rng, d)
            for q, t in ((np.concatenate([s, y]), np.concatenate([x, s])), (np.concatenate([y, s]), np.concatenate([s, x]))):
                kswgen._add_glb(pw, q, t, d - 1)  # the witness: one diagonal short
                for w in (d, d + 1, d + 20):
                    kswgen._add_glb(pb, q, t, w)
    batch, wit = kswgen.finish_glb(pb), kswgen.finish_glb(pw)
    # every task is a witness, by the oracle alone: a band one short of d scores strictly less, d, d + 1 and d + 20 score the same
    sc = kswlib.orc_global_batch_mt(p, *batch, nthreads=8)[0]["score"].reshape(-1, 3)
    short = kswlib.orc_global_batch_mt(p, *wit, nthreads=8)[0]["score"]
    assert len(short) == len(sc) == 64
    assert (short < sc[:, 0]).all() and (sc[:, 0] == sc[:, 1]).all() and (sc[:, 0] == sc[:, 2]).all()
    bands = _check(p, batch, what=f"{scoring}: ")
    assert (bands == batch[1]["w"]).all()  # the rule leaves these alone, so w says which kernel runs them
    # ... and the bands one short, where the kernels must lose what the oracle loses
    _check(p, wit, envs=({},), what=f"{scoring}, one short: ")


# ---- 4. the eight-lane split as the device executes it ----------------------------------------------------------------------------

PAIRS = tuple(range(1, 10)) + (15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)


def _prefix(p, q, t):
    """Sum of s0 - s1 over the pairs in front of every gap position 0..n (the quantity the lanes' parts are joined for)."""
    mat = np.asarray(p["mat"], dtype=np.int64).reshape(5, 5)
    q, t = q.astype(np.int64), t.astype(np.int64)
    d, n = len(q) - len(t), min(len(q), len(t))
    s0, s1 = (mat[t, q[:n]], mat[t, q[d:]]) if d > 0 else (mat[t[:n], q], mat[t[-d:], q])
    return np.concatenate([[0], np.cumsum(s0 - s1)])


def test_the_eight_lane_split_as_executed():
    rng = np.random.default_rng(8800)
    p = kswlib.make_params()
    pb, m, on_boundary = kswgen.PoolBuilder(kswlib.GLB_TASK), 0, 0
    for n in PAIRS:
        per = 8 * ((n + 63) // 64)  # pairs per lane
        bounds = [g * per for g in range(1, 8) if g * per <= n]
        xs = sorted({x for b in bounds for x in (b - 1, b, b + 1) if 0 <= x <= n} | {0, n // 2, n})
        for x in xs:
            for sign in (1, -1):
                s = kswgen.rand_seq(rng, n)
                ins = kswgen.rand_seq(rng, 3)
                if x >= 1:
                    ins[2] = (s[x - 1] + 1) & 3  # the pair in front of the gap matches on the main diagonal only ...
                if x < n:
                    ins[0] = (s[x] + 1) & 3      # ... and the pair behind it on the far corner's only
                long_, short = np.concatenate([s[:x], ins, s[x:]]), s.copy()
                m = m % 4 + 1  # 1..4 substitutions in front of the gap, eight apart: the band then moves with the bound's last unit
                for i in range(m):
                    if x - 2 - 8 * i >= 0:
                        short[x - 2 - 8 * i] = (short[x - 2 - 8 * i] + 2) & 3
                q, t = (long_, short) if sign > 0 else (short, long_)
                pre = _prefix(p, q, t)
                assert len(pre) == n + 1 and pre[x] == pre.max(), (n, x, sign)  # x is a best gap position
                on_boundary += x in bounds
                kswgen._add_glb(pb, q, t, 30)
    batch = kswgen.finish_glb(pb)
    tasks = batch[1]
    assert on_boundary >= 2 * 7 * 8 and len(tasks) < 2000
    assert set(tasks["q_off"] % 8) == set(range(8)) and set(tasks["t_off"] % 8) == set(range(8))  # packed back to back
    bands = _check(p, batch, envs=({},), what="split: ")
    past = tasks["tlen"] > gr.ROWS_CAP  # (two pair counts with the deletion: past the lane kernels' rows, so left at w)
    assert 0 < int(past.sum()) <= 48 and (bands[past] == 30).all() and (bands[~past] < 30).all() and len(set(bands[~past])) >= 4


def test_the_read_back_refuses_what_it_cannot_answer():
    pkg = load_package()
    rng = np.random.default_rng(1)
    p = kswlib.make_params()
    pool, tasks, words = kswgen.gen_glb_realistic(rng, 40)

    def refused(ctx, n):
        with pytest.raises(pkg.BmhError) as e:
            ctx.last_global_bands(n)
        assert e.value.code == pkg.BMH_E_ARG

    ctx = _ctx_with({})
    try:
        ctx.set_params(p)
        refused(ctx, 40)  # no launch yet
        ctx.global_batch(pool, tasks, words)
        for n in (39, 41, 0):  # not that launch's task count
            refused(ctx, n)
        assert np.array_equal(ctx.last_global_bands(40), gr.expected_bands(p, pool, tasks))
    finally:
        ctx.close()
    ctx = _ctx_with({"BMH_GLB_MODE": "wave"})  # no lane kernels, so no band pass
    try:
        ctx.set_params(p)
        ctx.global_batch(pool, tasks, words)
        refused(ctx, 40)
    finally:
        ctx.close()
