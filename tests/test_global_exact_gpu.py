"""global_narrow_kernel (csrc/global_narrow.hip): bands of 0..3 (bin 6) and 4..7 (bin 7) of the global dispatcher, each row on exactly
its 2w+1 cells, behind BMH_GLB_EXACT.

Every batch is compared field by field and CIGAR word by CIGAR word with
  * the oracle's ksw_global2 at the task's own w, and
  * the same call on a context with BMH_GLB_EXACT=0 (the bins as they were),
and the number of tasks the sort put into bins 6 and 7 (bmh_last_global_bin_counts) must be the one the rule restated in
glbbin_ref.py predicts: equal results alone would not show that a task ran on the new kernel.  Every assertion is an equality.

The contexts under test set BMH_GLB_EXACT themselves (7, and 3 where said), so the cases do not move with the default."""
import importlib

import numpy as np
import pytest

import devcalls as dc
import glbband_ref as gr
import glbbin_ref as br
import kswgen
import kswlib
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu


def _tg():
    return importlib.import_module(load_package().__name__ + ".taskgen")


def _same_cigars(res, cig, res0, cig0, tasks, what):
    assert (res == res0).all(), f"{what}results differ from BMH_GLB_EXACT=0; first at {np.nonzero(res != res0)[0][0]}"
    for k, t in enumerate(tasks):
        o, n = int(t["cigar_off"]), int(res[k]["n_cigar"])
        if 0 < n <= int(t["cigar_cap"]):
            assert np.array_equal(cig[o:o + n], cig0[o:o + n]), f"{what}task {k}: CIGAR words differ from BMH_GLB_EXACT=0"


def _check(p, batch, narrow=True, exact=7, what="", bands=False):
    """The batch on a context with the exact bins on: the oracle's results, the predicted bin counts; then with BMH_GLB_EXACT=0: the
    same results and words, nothing in bins 6 and 7.  Returns (bins, bands run on) of the tasks as predicted."""
    pool, tasks, words = batch
    assert not (tasks["tlen"].astype(np.int64) > tasks["qlen"].astype(np.int64) + tasks["w"]).any()  # (the reference's traceback is undefined there)
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    env = {"BMH_GLB_EXACT": str(exact), **({} if narrow else {"BMH_GLB_NARROW": "0"})}
    bins, ws = br.expected_bins(p, pool, tasks, narrow=narrow, exact=exact)
    expect = np.bincount(bins, minlength=8)
    ctx = _ctx_with(env)
    try:
        ctx.set_params(p)
        res, cig = ctx.global_batch(pool, tasks, words)
        counts = ctx.last_global_bin_counts()
        print(f"{what}{env}: bins {counts.tolist()}")
        dc.assert_glb(res, cig, want, wcig, tasks, f"{what}{env}: ")
        assert (counts == expect).all(), f"{what}{env}: bin counts {counts.tolist()}, the rule gives {expect.tolist()}"
        if bands:
            assert np.array_equal(ctx.last_global_bands(len(tasks)), gr.expected_bands(p, pool, tasks))
    finally:
        ctx.close()
    ctx = _ctx_with({**env, "BMH_GLB_EXACT": "0"})
    try:
        ctx.set_params(p)
        res0, cig0 = ctx.global_batch(pool, tasks, words)
        c0 = ctx.last_global_bin_counts()
        assert c0[6] == 0 and c0[7] == 0 and c0[5] == expect[5] + expect[6] + expect[7] and (c0[:5] == expect[:5]).all(), c0.tolist()
        _same_cigars(res, cig, res0, cig0, tasks, what)
    finally:
        ctx.close()
    return bins, ws


# ---- 1. exhaustive small shapes ---------------------------------------------------------------------------------------------------

def _below_set(letters, maxlen):
    """Every (q, t) with qlen > tlen at every w below qlen - tlen: the band does not reach the last cell and the score is the
    reference's MINUS_INF (with tlen > qlen the reference's traceback is undefined at such a band)."""
    import itertools
    seqs = [np.array(s, dtype=np.uint8) for n in range(1, maxlen + 1) for s in itertools.product(range(letters), repeat=n)]
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for q in seqs:
        for t in seqs:
            for w in range(0, len(q) - len(t)):
                kswgen._add_glb(pb, q, t, w)
    return kswgen.finish_glb(pb)


@pytest.fixture(scope="module")
def small_sets():
    full, below = gr.exhaustive_set(2, 5, 7), _below_set(2, 5)
    assert len(full[1]) == 26576 and len(below[1]) == 2088
    assert set(full[1]["w"]) == set(range(8)) and set(below[1]["w"]) == set(range(4))
    return full, below


@pytest.mark.parametrize("scoring", list(gr.SCORINGS))
def test_every_small_pair_at_every_band(small_sets, scoring):
    """Every pair of sequences of up to five bases of two letters at every band 0..7 (w >= |delta|), and at every band below |delta|
    where the reference is defined; with the band pass and, without it, on the tasks' own w."""
    p = kswlib.make_params(**gr.SCORINGS[scoring])
    full, below = small_sets
    for narrow in (True, False):
        bins, ws = _check(p, full, narrow=narrow, what=f"{scoring}/full: ")
        assert set(bins) == {6, 7} and (set(ws) == set(range(8)) if not narrow else set(ws) >= {0, 1, 2, 3, 4})
        bins, ws = _check(p, below, narrow=narrow, what=f"{scoring}/below: ")
        assert set(bins) == {6} and (ws == below[1]["w"]).all()  # the rule leaves w < |delta| alone
    want = kswlib.orc_global_batch_mt(p, *below, nthreads=8)[0]
    assert (want["score"] < -(1 << 29)).all()


# ---- 2. band boundaries -----------------------------------------------------------------------------------------------------------

def _subst(rng, s, k):
    t = s.copy()
    for x in rng.choice(len(s), size=k, replace=False):
        t[x] = (t[x] + 1 + rng.integers(0, 3)) & 3
    return t


@pytest.mark.parametrize("exact", [7, 3])
def test_narrowing_onto_every_band_up_to_eight(exact):
    """Equal lengths with k substitutions narrow onto floor((5k - 12) / 3) = 1, 2, 4, 6, 7, 9 for k = 3..8, one gap of d bases and no
    substitution onto d: every band 0..8 is reached, 3 | 4 and 7 | 8 from both sides, and 8 lands in bin 5."""
    rng = np.random.default_rng(7100 + exact)
    p = kswlib.make_params()
    L, w = 150, 100
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for rep in range(3):
        for k in range(0, 9):
            q = kswgen.rand_seq(rng, L)
            kswgen._add_glb(pb, q, _subst(rng, q, k), w)
        for d in range(1, 10):
            q = kswgen.rand_seq(rng, L)
            x = int(rng.integers(20, L - 20))
            kswgen._add_glb(pb, q, np.concatenate([q[:x], q[x + d:]]), w)                          # an insertion of d bases
            kswgen._add_glb(pb, np.concatenate([q[:x], q[x + d:]]), q, w, want_cigar=rep != 1)     # a deletion
    batch = kswgen.finish_glb(pb)
    bins, ws = _check(p, batch, exact=exact, what=f"exact {exact}: ", bands=True)
    assert set(range(9)) <= set(ws)
    for band in range(9):
        on = bins[ws == band]
        assert len(on) >= 2 and (on == (6 if band <= 3 else 7 if band <= 7 and exact == 7 else 5)).all(), (band, on)


# ---- 3. head and tail rows --------------------------------------------------------------------------------------------------------

def _near(rng, q, tl):
    """A target of tl bases close to q: q cut or extended at a random place."""
    if tl <= len(q):
        x = int(rng.integers(0, tl + 1))
        return np.concatenate([q[:x], q[x + len(q) - tl:]])
    x = int(rng.integers(0, len(q) + 1))
    return np.concatenate([q[:x], kswgen.rand_seq(rng, tl - len(q)), q[x:]])


@pytest.mark.parametrize("W", range(8))
def test_head_and_tail_rows(W):
    """On the tasks' own w = W (BMH_GLB_NARROW=0) and with the band pass: queries of 1..2W+2 bases, where every row is a boundary row;
    tlen = 1; |delta| = W in both signs with the optimum on the outermost diagonal; tlen = qlen +- 1..W."""
    rng = np.random.default_rng(7300 + W)
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for ql in range(1, 2 * W + 3):
        q = kswgen.rand_seq(rng, ql)
        for tl in sorted({1} | set(range(max(1, ql - W), ql + W + 1))):
            if tl <= ql + W:  # (the reference's traceback is defined)
                kswgen._add_glb(pb, q, _near(rng, q, tl), W)
                kswgen._add_glb(pb, q, kswgen.rand_seq(rng, tl), W, want_cigar=tl % 3 != 0)
    for ls in (9, 40, 130):  # the optimum on the outermost diagonal, either side (as test_global_band_exact_gpu.py builds it)
        s, x, y = kswgen.rand_seq(rng, ls), kswgen.rand_seq(rng, W), kswgen.rand_seq(rng, W)
        for q, t in ((np.concatenate([s, y]), np.concatenate([x, s])), (np.concatenate([y, s]), np.concatenate([s, x]))):
            kswgen._add_glb(pb, q, t, W)
        for d in range(1, W + 1):  # tlen = qlen +- d
            q = kswgen.rand_seq(rng, ls + W)
            kswgen._add_glb(pb, q, _near(rng, q, len(q) - d), W)
            kswgen._add_glb(pb, q, _near(rng, q, len(q) + d), W)
    batch = kswgen.finish_glb(pb)
    p = kswlib.make_params()
    bins, ws = _check(p, batch, narrow=False, what=f"W={W} own: ")
    assert (ws == W).all() and (bins == (6 if W <= 3 else 7)).all()
    _check(p, batch, narrow=True, what=f"W={W} narrowed: ")
    _check(kswlib.make_params(**gr.SCORINGS["asymmetric"]), batch, narrow=False, what=f"W={W} asymmetric: ")


def test_rows_at_the_slabs_capacity_and_past_it():
    """tlen == rows_cap (512) runs in the exact bins, tlen == 513 goes to the wave kernel (bin 2)."""
    rng = np.random.default_rng(7400)
    p = kswlib.make_params()
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for W in (0, 2, 3, 4, 7):
        for tl in (gr.ROWS_CAP, gr.ROWS_CAP + 1, gr.ROWS_CAP - 1):
            t = kswgen.rand_seq(rng, tl)
            kswgen._add_glb(pb, _near(rng, t, tl - W), t, W)
            kswgen._add_glb(pb, _subst(rng, t, 3), t, W)
    batch = kswgen.finish_glb(pb)
    bins, ws = _check(p, batch, narrow=False, what="rows: ")
    past = batch[1]["tlen"] > gr.ROWS_CAP
    assert past.sum() == 10 and (bins[past] == 2).all() and np.isin(bins[~past], (6, 7)).all()
    _check(p, batch, narrow=True, what="rows, narrowed: ")


# ---- 4. waves ---------------------------------------------------------------------------------------------------------------------

def _one_band(rng, pb, n, W, lens=(20, 60)):
    for _ in range(n):
        q = kswgen.rand_seq(rng, int(rng.integers(lens[0], lens[1] + 1)))
        d = int(rng.integers(-W, W + 1))
        t = _subst(rng, _near(rng, q, max(1, len(q) + d)), int(rng.integers(0, 3)))
        kswgen._add_glb(pb, q, t, W, want_cigar=rng.random() < 0.9)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batches_of_one_band(n):
    rng = np.random.default_rng(7500 + n)
    p = kswlib.make_params()
    for W in (0, 1, 3, 4, 6, 7):
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        _one_band(rng, pb, n, W)
        bins, ws = _check(p, kswgen.finish_glb(pb), narrow=False, what=f"n={n} W={W}: ")
        assert (ws == W).all() and len(set(bins)) == 1


@pytest.mark.parametrize("mix", [(1, 2), (0, 3), (4, 5), (0, 1, 2), (5, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7), (2, 3, 4, 5)])
def test_a_wave_of_mixed_bands(mix):
    """One 64-task group that holds two, three or four bands (the seam pass), alone and behind a full wave of the widest band."""
    rng = np.random.default_rng(7600 + sum(1 << w for w in mix))
    p = kswlib.make_params()
    for lead in (0, 64):
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        _one_band(rng, pb, lead, max(mix))
        share = [64 // len(mix)] * len(mix)
        share[0] += 64 - sum(share) - (3 if lead == 0 else 0)  # (alone: 61 tasks, a wave with idle lanes at its end)
        for W, k in zip(mix, share):
            _one_band(rng, pb, k, W)
        batch = kswgen.finish_glb(pb)
        perm = rng.permutation(len(batch[1]))  # the sort, not the input order, brings the bands together
        batch = (batch[0], batch[1][perm], batch[2])
        bins, ws = _check(p, batch, narrow=False, what=f"mix {mix}, lead {lead}: ")
        for b in set(bins):
            waves = br.narrow_waves(bins, ws, batch[1]["tlen"], int(b))
            print(f"mix {mix}, lead {lead}: bin {b} waves {waves}")
        assert set(ws) == set(mix)
        if all(w <= 3 for w in mix) or all(w >= 4 for w in mix):
            assert max(len(x) for x in br.narrow_waves(bins, ws, batch[1]["tlen"], int(bins[0]))) == len(mix)


def test_one_band_from_20_to_300_rows():
    rng = np.random.default_rng(7700)
    p = kswlib.make_params()
    for W in (2, 5):
        pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
        for L in rng.permutation(np.arange(20, 301, 2)):
            _one_band(rng, pb, 1, W, lens=(int(L), int(L)))
        bins, ws = _check(p, kswgen.finish_glb(pb), narrow=False, what=f"20-300 rows, W={W}: ")
        assert (ws == W).all()


# ---- 5. task list edges -----------------------------------------------------------------------------------------------------------

def test_a_sparse_order_on_the_device():
    """bmh_global_batch_device with a permuted d_order of 3 000 entries over 10 000 records.  Every bin's kernel reads its task count
    from the device (the sort's counters): always smaller than the n it is launched with."""
    rng = np.random.default_rng(7800)
    p = kswlib.make_params()
    pool, tasks, words = _tg().generate_global(10000, "150bp", seed=941, wspread=32)
    order = rng.permutation(len(tasks))[:3000].astype(np.uint32)
    want, wcig, _ = kswlib.orc_global_batch_mt(p, pool, tasks, words, nthreads=8)
    rows_cap = min(int(tasks["qlen"].max()) + 2 * int(p["w"]) + 64, gr.ROWS_CAP)  # of a device-resident launch: from the capacity hint
    expect = np.bincount(br.expected_bins(p, pool, tasks[order], rows_cap=rows_cap)[0], minlength=8)
    assert expect[6] > 1000 and expect[7] > 500 and expect[6] + expect[7] < len(order)
    got = {}
    for exact in ("7", "0"):
        ctx = _ctx_with({"BMH_GLB_EXACT": exact})
        try:
            ctx.set_params(p)
            ctx.set_qcap(int(tasks["qlen"].max()))
            g = dc.Glb(pool, tasks, words, order)
            g.n = len(order)
            g.run(ctx)
            ctx.sync()
            counts = ctx.last_global_bin_counts()
            g.n = len(tasks)
            got[exact] = g.result()
        finally:
            ctx.close()
        if exact == "7":
            assert (counts == expect).all(), (counts.tolist(), expect.tolist())
        else:
            assert counts[6] == 0 and counts[7] == 0 and counts.sum() == len(order)
    res, cig = got["7"]
    dc.assert_glb(res[order], cig, want[order], wcig, tasks[order], "sparse order: ")
    _same_cigars(res[order], cig, got["0"][0][order], got["0"][1], tasks[order], "sparse order: ")
    rest = np.setdiff1d(np.arange(len(tasks)), order)
    assert (res[rest].view(np.uint8) == res[rest].view(np.uint8)[0]).all(), "a record outside the order was written"


# ---- 6. CIGAR ---------------------------------------------------------------------------------------------------------------------

def _cigar_batch(rng):
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    for W in range(8):
        _one_band(rng, pb, 12, W, lens=(30, 90))
    return kswgen.finish_glb(pb)


def _with_caps(batch, caps):
    pool, tasks, _ = batch
    tasks = tasks.copy()
    tasks["cigar_cap"] = caps
    off = 0
    for t in tasks:
        t["cigar_off"] = off
        off += int(t["cigar_cap"])
    return pool, tasks, off


def test_cigar_capacities():
    """No CIGAR wanted; a capacity of exactly n_cigar; one word too few, which is BMH_E_CIGAR_CAP as with the switch off."""
    pkg = load_package()
    rng = np.random.default_rng(7900)
    p = kswlib.make_params()
    batch = _cigar_batch(rng)
    n_cigar = kswlib.orc_global_batch_mt(p, *_with_caps(batch, batch[1]["qlen"].astype(np.int64) + batch[1]["tlen"] + 2), nthreads=4)[0]["n_cigar"]
    assert n_cigar.max() >= 3 and (n_cigar >= 1).all()
    _check(p, _with_caps(batch, 0), narrow=False, what="want == 0: ")
    _check(p, _with_caps(batch, n_cigar), narrow=False, what="cap == n_cigar: ")
    for victim in np.nonzero(n_cigar >= 2)[0][[0, -1]]:  # one in bin 6, one in bin 7
        caps = n_cigar.copy()
        caps[victim] -= 1
        short = _with_caps(batch, caps)
        for exact in ("7", "0"):
            ctx = _ctx_with({"BMH_GLB_EXACT": exact, "BMH_GLB_NARROW": "0"})
            try:
                ctx.set_params(p)
                with pytest.raises(pkg.BmhError) as e:
                    ctx.global_batch(*short)
                assert e.value.code == pkg.BMH_E_CIGAR_CAP, (exact, e.value.code)
            finally:
                ctx.close()


def test_the_counts_read_back_refuses_what_it_cannot_answer():
    pkg = load_package()
    rng = np.random.default_rng(2)
    p = kswlib.make_params()
    pool, tasks, words = kswgen.gen_glb_realistic(rng, 40)
    ctx = _ctx_with({"BMH_GLB_EXACT": "7"})
    try:
        ctx.set_params(p)
        with pytest.raises(pkg.BmhError) as e:
            ctx.last_global_bin_counts()  # no launch yet
        assert e.value.code == pkg.BMH_E_ARG
        ctx.global_batch(pool, tasks, words)
        counts = ctx.last_global_bin_counts()
        assert counts.sum() == 40 and (counts == br.expected_counts(p, pool, tasks)).all()
        epool, etasks = kswgen.gen_ext_realistic(rng, 64)
        ctx.extend_batch(epool, etasks)  # another sort has used the workspace
        with pytest.raises(pkg.BmhError) as e:
            ctx.last_global_bin_counts()
        assert e.value.code == pkg.BMH_E_ARG
    finally:
        ctx.close()


# ---- 7. the generator's tasks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,n", [("150bp", 3000), ("mixed100-300", 2000)])
def test_generator_tasks(shape, n):
    p = kswlib.make_params()
    batch = _tg().generate_global(n, shape, seed=939, wspread=32)
    assert len(batch[1]) == n
    for exact in (7, 3):
        bins, ws = _check(p, batch, exact=exact, what=f"{shape}, exact {exact}: ", bands=True)
        assert (bins == 6).sum() > n // 20 and ((bins == 7).sum() > n // 20) == (exact == 7)
