"""The lane kernels' sequence stream (csrc/seq_stream.h: batches of clamped, unconditional loads, one wait per batch) at the lengths
where its clamps and masks change: sequences shorter than a dword, lengths around one, two and three refills of 64 rows, and a task
whose sequences are the last bytes of the pool.  Every result is compared with the oracle, field by field and CIGAR word by word;
the global cases also assert the bin -- and with it the kernel -- the tasks ran in (bmh_last_global_bin_counts)."""
import numpy as np
import pytest

import kswgen
import kswlib
import glbband_ref as gr
from kswlib import BMH_F_QREV, BMH_F_TREV, BMH_F_TPAC, EXT_TASK
from test_global_exact_gpu import _check, _near, _subst
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

GROUPS = [range(1, 10), range(60, 69), range(124, 133), range(188, 197)]
# band -> bin of the global dispatcher: global_narrow_kernel<0> / <4>, global_lane_kernel<32> / <64> / <96> / <128>
BIN_OF = {**{w: 6 for w in range(4)}, **{w: 7 for w in range(4, 8)}, 8: 5, 16: 0, 33: 3, 50: 1}


def _global_batch(w, seed):
    """Every (qlen, tlen) of one length group with tlen <= qlen + w (where the reference's traceback is defined), equal lengths among
    them; the target a copy of the query with a cut or an insert and up to two substitutions; every third task without a CIGAR.  The
    last task's query and target are the last bytes of the pool."""
    rng = np.random.default_rng(seed)
    pb = kswgen.PoolBuilder(kswlib.GLB_TASK)
    k = 0
    for grp in GROUPS:
        for ql in grp:
            q = kswgen.rand_seq(rng, ql)
            for tl in grp:
                if tl > ql + w:
                    continue
                t = _near(rng, q, tl)
                kswgen._add_glb(pb, q, _subst(rng, t, min(int(rng.integers(0, 3)), tl)), w, want_cigar=k % 3 != 0)
                k += 1
    pool, tasks, words = kswgen.finish_glb(pb)
    last = tasks[-1]
    assert int(last["t_off"]) + int(last["tlen"]) == len(pool) - 8 and int(last["q_off"]) + int(last["qlen"]) == int(last["t_off"])
    return pool[:-8].copy(), tasks, words  # (the builder's eight bytes of padding go)


@pytest.mark.parametrize("w", sorted(BIN_OF))
def test_global_tasks_around_every_refill(w):
    batch = _global_batch(w, 8100 + w)
    lens = set(zip(batch[1]["qlen"].tolist(), batch[1]["tlen"].tolist()))
    assert all((n, n) in lens for g in GROUPS for n in g) and any(a != b for a, b in lens)
    assert (batch[1]["cigar_cap"] == 0).any() and (batch[1]["cigar_cap"] > 0).any()
    p = kswlib.make_params()
    bins, ws = _check(p, batch, narrow=False, what=f"w={w}: ")
    assert (ws == w).all() and (bins == BIN_OF[w]).all(), (w, sorted(set(bins.tolist())))
    _check(kswlib.make_params(**gr.SCORINGS["asymmetric"]), batch, narrow=False, what=f"w={w} asymmetric: ")


# ---- extension ---------------------------------------------------------------------------------------------------------------------

FLANKS = [*range(1, 10), 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
TARGETS = [1, 2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 130]


def _ext_batch(seed):
    """Every flank length against every target length, all four combinations of the reversed flags; the query a copy of the
    target's head with a few substitutions, so that rows run on to the target's end."""
    rng = np.random.default_rng(seed)
    pb = kswgen.PoolBuilder(EXT_TASK)
    for ql in FLANKS:
        for tl in TARGETS:
            for qrev in (False, True):
                for trev in (False, True):
                    t = kswgen.rand_seq(rng, tl)
                    q = np.concatenate([t, kswgen.rand_seq(rng, max(0, ql - tl))])[:ql].copy()
                    q = _subst(rng, q, min(ql // 16, 3)) if ql > 1 else q
                    qo, to = pb.put(q, qrev), pb.put(t, trev)
                    flags = (BMH_F_QREV if qrev else 0) | (BMH_F_TREV if trev else 0)
                    pb.tasks.append((qo, to, ql, tl, int(rng.integers(5, 60)), int(rng.choice([100, 100, 11, 3])), 5, flags, 0))
    pool, tasks = pb.finish()
    return pool[:-8].copy(), tasks  # the last target, stored reversed, ends where the pool ends


def test_extension_flanks_and_targets_around_every_refill():
    pool, tasks = _ext_batch(8200)
    assert len(tasks) == len(FLANKS) * len(TARGETS) * 4
    last = tasks[-1]
    assert last["flags"] & BMH_F_TREV and int(last["t_off"]) == len(pool) - 1
    p = kswlib.make_params()
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=8)
    assert (want["score"] > 30).sum() > len(tasks) // 4  # many run long
    for env in ({"BMH_EXT_MODE": "lane"}, {}):
        ctx = _ctx_with(env)
        try:
            got = ctx.extend_batch(pool, tasks)
        finally:
            ctx.close()
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{env}: {len(bad)} differ; first {tasks[bad[0]]}: gpu={got[bad[0]]} oracle={want[bad[0]]}"


def test_a_target_in_the_2bit_reference_beside_pool_targets():
    """BMH_F_TPAC targets keep their base-by-base path: one such task per wave of pool tasks, forward and reversed."""
    rng = np.random.default_rng(8300)
    l_pac = 1003
    bases = rng.integers(0, 4, l_pac, dtype=np.uint8)
    pad = np.concatenate([bases, np.zeros((-l_pac) % 4 + 4, np.uint8)])
    q4 = pad[: (len(pad) // 4) * 4].reshape(-1, 4)
    pac = (q4[:, 0] << 6 | q4[:, 1] << 4 | q4[:, 2] << 2 | q4[:, 3]).astype(np.uint8)
    pool, tasks = _ext_batch(8301)
    pool = np.concatenate([pool, np.zeros(8, np.uint8)])
    tasks = tasks[(tasks["qlen"] >= 31) & (tasks["qlen"] <= 65)].copy()
    assert len(tasks) > 128
    for k, (pos, tl, trev) in zip(range(5, len(tasks), 40), [(100, 70, False), (400, 130, True), (700, 3, False), (900, 66, True)]):
        t = tasks[k]
        fwd = bases[pos:pos + tl]
        q = _subst(rng, np.concatenate([fwd if not trev else fwd[::-1], kswgen.rand_seq(rng, 64)])[:int(t["qlen"])].copy(), 2)
        qs = q[::-1] if t["flags"] & BMH_F_QREV else q
        pool[int(t["q_off"]) - (len(q) - 1 if t["flags"] & BMH_F_QREV else 0):][:len(q)] = qs
        t["t_off"], t["tlen"] = (pos + tl - 1 if trev else pos), tl
        t["flags"] = (int(t["flags"]) & BMH_F_QREV) | BMH_F_TPAC | (BMH_F_TREV if trev else 0)
    assert (tasks["flags"] & BMH_F_TPAC != 0).sum() == 4
    p = kswlib.make_params()
    want, _ = kswlib.orc_extend_batch(p, pool, tasks, nthreads=4, pac=pac, l_pac=l_pac)
    ctx = _ctx_with({"BMH_EXT_MODE": "lane"})
    try:
        ctx.set_pac(pac, l_pac)
        got = ctx.extend_batch(pool, tasks)
    finally:
        ctx.close()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} differ; first {tasks[bad[0]]}: gpu={got[bad[0]]} oracle={want[bad[0]]}"
    assert (want[tasks["flags"] & BMH_F_TPAC != 0]["score"] > 0).all()
