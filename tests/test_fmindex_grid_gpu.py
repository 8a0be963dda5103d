"""One batch past every grid cap of the FM-index kernels, on the library's own choices (no BMH_SMEM_* variable set): the
grid-stride loops of smem_kernel (which the library picks, in its five-wave build, above 262 144 reads), smem_order_count,
smem_order_place, sa_of_intervals_kernel and sa_kernel run their second trip only above the sizes asserted below -- the
constants of smem_impl and bmh_sa_batch.  The batch is 5 200 distinct short reads, each 64 times over in a fixed
shuffled order, so the oracle runs 5 200 times and its answer is expanded by index; the comparison is flat."""
import numpy as np
import pytest

import kswlib
import tinyindex as ti
from test_fmindex_cpu import _intv_len, _orc_calls, fixture_reads
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

N_DISTINCT, COPIES = 5200, 64
NONE = np.uint64(0xffffffffffffffff)
_batch = {}


def _big_batch():
    """(distinct reads, oracle answer per distinct read, index of the distinct read behind every read of the batch)"""
    if not _batch:
        cb, keep = kswlib.golden_fmindex()[:2]  # (keep holds the arrays cb points into)
        distinct = fixture_reads(229, N_DISTINCT, [20, 24, 32, 40, 48, 60], [0.0, 0.02, 0.12])
        o = kswlib.smem_option_set("fixture")
        want = [_orc_calls(cb, o, rd) for rd in distinct]
        order = np.random.default_rng(233).permutation(np.repeat(np.arange(N_DISTINCT), COPIES))
        _batch["v"] = distinct, want, order
    return _batch["v"]


def _flat(per_read):
    """per-read (calls, intervals) -> (calls per read, call fields [n, 5], intervals per read, intervals) in batch order"""
    cn = np.array([len(c) for c, _ in per_read])
    inn = np.array([len(i) for _, i in per_read])
    # (joined as bytes: np.concatenate takes seconds over 332 800 small record arrays)
    calls = np.frombuffer(b"".join([c.tobytes() for c, _ in per_read]), dtype=kswlib.SMEM_CALL)
    intv = np.frombuffer(b"".join([i.tobytes() for _, i in per_read]), dtype=kswlib.SMEM_INTV)
    return cn, np.stack([calls[f].astype(np.int64) for f in ("x", "min_intv", "ret", "n", "first")], 1), inn, intv


def test_smem_and_seed_batch_past_every_grid_cap(monkeypatch):
    for k in ("BMH_SMEM_KERNEL", "BMH_SMEM_WAVES", "BMH_SMEM_LANES", "BMH_SMEM_EMIT", "BMH_SMEM_INIT_CAP"):
        monkeypatch.delenv(k, raising=False)
    cb, keep, raw, opt, _, per, sa_k, sa_pos = kswlib.golden_fmindex()
    distinct, want, order = _big_batch()
    reads = [distinct[d] for d in order]
    wcn, wcalls, winn, wintv = _flat([want[d] for d in order])
    # past each cap, on the expectation (the constants are smem_impl's)
    assert len(reads) == N_DISTINCT * COPIES > 1024 * 5 * 64  # smem_kernel<5>'s grid of 5 120 waves x 64 lanes
    assert len(reads) > 4 * 1024 * 64 and len(reads) > 128 * 1024  # ... which is the kernel the library picks here
    assert len(wcalls) > 2048 * 256                            # smem_order_count / smem_order_place
    assert len(wintv) > 4096 * 256                             # sa_of_intervals_kernel
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    o = kswlib.smem_option_set("fixture")
    gcn, gcalls, ginn, gintv = _flat(ctx.smem_batch(o, reads))
    assert (gcn == wcn).all() and (ginn == winn).all()
    assert (gcalls == wcalls).all()
    assert (gintv == wintv).all()
    # ---- the same batch with the look-ups
    got, offs, pos = ctx.seed_batch(o, 50, reads)
    scn, scalls, sinn, sintv = _flat(got)
    assert (scn == wcn).all() and (sinn == winn).all() and (scalls == wcalls).all() and (sintv == wintv).all()
    so = np.concatenate(offs)
    look = (_intv_len(wintv) >= int(o["min_seed_len"])) & (wintv["x2"] <= np.uint64(50))
    assert ((so != NONE) == look).all()
    x2 = wintv["x2"][look].astype(np.int64)
    assert int(x2.sum()) == len(pos) and look.sum() > 100_000
    # every looked-up interval's positions, gathered flat: pos[so + 0 .. so + x2) against sa_batch of rows x0 .. x0 + x2
    rep = np.repeat(np.arange(len(x2)), x2)
    within = np.arange(len(rep)) - np.repeat(np.cumsum(x2) - x2, x2)
    have = pos[so[look].astype(np.int64)[rep] + within]
    keys = wintv["x0"][look][rep] + within.astype(np.uint64)
    ukeys, inv = np.unique(keys, return_inverse=True)
    assert (have == ctx.sa_batch(ukeys)[inv]).all()
    assert (ctx.sa_batch(ukeys[::97]) == kswlib.orc_sa(cb, ukeys[::97])).all()
    ctx.close()


def test_sa_batch_past_its_grid_cap():
    """2 200 000 keys > 8192 x 256 on the 2 000-row tiny index: every row once and uniform draws, against the plain sort"""
    raw, sa = ti.shape("rand_1000")
    rows = ti.sa_rows(sa)
    rng = np.random.default_rng(239)
    n = 2_200_000
    assert n > 8192 * 256
    ks = np.concatenate([np.arange(raw[2] + 1), rng.integers(0, raw[2] + 1, n - raw[2] - 1)]).astype(np.uint64)
    rng.shuffle(ks)
    ctx = _ctx_with({})
    ctx.set_bwt(*raw)
    assert (ctx.sa_batch(ks) == rows[ks.astype(np.int64)]).all()
    ctx.close()
