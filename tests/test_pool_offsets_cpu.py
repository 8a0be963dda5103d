"""tests/bigpool.py keeps its contract, and the checkers are 64-bit clean: the oracle (and, where it is built, the compiled
reference) on the LARGE host pool returns the small pool's results at every placement, and the same tasks with their offsets cut
to 32 bits do not -- so a GPU mismatch in tests/test_pool_offsets_gpu.py can be blamed on the GPU side, and its inputs discriminate.
The large pools are np.zeros of up to 8 GiB: lazily mapped, only the pages written or read are ever touched."""
import numpy as np
import pytest

import bigpool as bp
import kswlib

P = kswlib.make_params()
HAS_REV = {"ext": True, "glb": False, "sw": True, "seed": False}   # (ksw_global2 tasks and fused seeds carry no REV flags)


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(4321)
    return {"ext": bp.ext_batch(rng, n_side=700, long_targets=24), "glb": bp.glb_batch(rng), "sw": bp.sw_batch(rng, P),
            "seed": bp.seed_batch(rng)}


def _oracle(kind, pool, tasks, b):
    if kind == "ext":
        return (kswlib.orc_extend_batch(P, pool, tasks, nthreads=4)[0],)
    if kind == "seed":
        return (kswlib.orc_seedext_batch(P, pool, tasks, nthreads=4)[0],)
    if kind == "sw":
        return (kswlib.orc_sw_batch(P, pool, tasks, nthreads=4)[0],)
    res, cig, _ = kswlib.orc_global_batch_mt(P, pool, tasks, b.words, nthreads=4)
    return res, cig


def _seqs(kind, pool, t):
    if kind == "sw":
        return kswlib.sw_task_seqs(pool, t)
    if kind == "seed":
        qo, to = int(t["q_off"]), int(t["t_off"])
        return pool[qo:qo + int(t["l_query"])], pool[to:to + int(t["wlen"])]
    return kswlib.task_seqs(pool, t)


@pytest.mark.parametrize("kind", ["ext", "glb", "sw", "seed"])
def test_relocated_views_decode_to_the_same_sequences_and_meet_the_caps(batches, kind):
    b = batches[kind]
    if kind in ("ext", "sw"):   # every flag combination occurs among the views
        for fam in (bp.FAM_T, bp.FAM_Q):
            f = b.tasks["flags"][b.fam == fam] & (kswlib.BMH_F_QREV | kswlib.BMH_F_TREV)
            assert set(f.tolist()) == {0, 1, 2, 3}
    for pl in bp.PLACEMENTS:
        big, moved = b.relocate(pl)
        assert len(big) == b.total(pl) and (moved["q_off"] >= b.base(pl)).all()
        for k in range(len(moved)):
            for x, y in zip(_seqs(kind, b.pool, b.tasks[k]), _seqs(kind, big, moved[k])):
                assert np.array_equal(x, y), f"{pl}: task {k} decodes differently after relocation"
        c = b.census(pl)
        if bp.BOUNDARY[pl] is not None:
            bp.assert_caps(c, HAS_REV[kind], f"{kind} {pl}: ")
            assert c["ord"]["across"] == 0       # S lies between the two halves: every straddler is a view
        else:
            assert c["ord"]["below"] == 0 and (moved["q_off"] & np.uint64(1 << 31)).all()
        # the decoy: a different valid base code wherever a truncated offset would land, nothing but zeros elsewhere
        base, n = b.base(pl), len(b.pool)
        segs = b.segments(pl)
        assert len(segs) >= 2 and sum(len(r) for _, r in segs[:-1]) > 0
        for off, run in segs[:-1]:
            assert (run < 4).all() and np.array_equal(big[off:off + len(run)], run)
        for m in bp.MASKS[pl]:
            x = np.arange(max(base, m + 1), base + n, dtype=np.int64)
            assert (big[x & m] != big[x]).all() and (big[x & m] < 4).all()
        lo = min(o for o, _ in segs)
        assert not big[max(0, lo - 4096):lo].any() and not big[base + n:].any()


def test_a_tpac_target_is_a_coordinate_and_stays():
    t = np.zeros(2, kswlib.EXT_TASK)
    t["q_off"], t["t_off"], t["flags"] = 5, 7, (kswlib.BMH_F_TPAC, 0)
    m = bp.shifted(t, bp.TWO32)
    assert m["q_off"].tolist() == [bp.TWO32 + 5] * 2 and m["t_off"].tolist() == [7, bp.TWO32 + 7]


@pytest.mark.parametrize("kind", ["ext", "glb", "sw", "seed"])
def test_oracle_on_the_large_pool_equals_the_small_pool_and_truncated_offsets_do_not(batches, kind):
    b = batches[kind]
    want = _oracle(kind, b.pool, b.tasks, b)
    for pl in bp.PLACEMENTS:
        big, moved = b.relocate(pl)
        got = _oracle(kind, big, moved, b)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), f"{kind} {pl}: the oracle on the large pool differs from the small pool"
        for m in bp.MASKS[pl]:   # a reader that drops the high word: in bounds thanks to the decoy, and wrong
            bad = _oracle(kind, big, b.truncated(pl, m), b)[0]
            hit = (b.truncated(pl, m)["q_off"] != moved["q_off"]) | (b.truncated(pl, m)["t_off"] != moved["t_off"])
            differ = bad != want[0]
            views = b.fam != bp.ORD
            print(f"{kind} {pl} mask {m:#x}: {int(differ.sum())} of {int(hit.sum())} truncated tasks change their result, "
                  f"{int((differ & views).sum())} of {int((hit & views).sum())} views")
            # Which views a dropped high word moves: all of them where the whole block lies above 2^32; at a straddling placement
            # those whose base 0 lies above the boundary -- the reversed ones, a quarter of each family at least.  (A forward
            # view starts below it: what it is there to catch is 32-bit arithmetic AFTER the start offset, which an oracle
            # run cannot imitate.)  Nearly every moved task must change: unrelated bases score differently.
            assert differ[hit].mean() > 0.9 and (differ & views).sum() >= 0.9 * (hit & views).sum()
            if bp.BOUNDARY[pl] is None:
                assert (hit & views).sum() == views.sum() >= 2 * bp.MIN_VIEWS
            elif HAS_REV[kind]:
                assert (hit & views).sum() >= bp.MIN_VIEWS // 2
            assert not differ[~hit].any()
        del big


@pytest.mark.ref
@pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built")
def test_compiled_reference_on_the_large_pool_equals_the_small_pool(batches):
    for pl in bp.PLACEMENTS:
        b = batches["ext"]
        sel = np.nonzero(b.fam != bp.ORD)[0].tolist() + list(range(0, len(b.tasks), 7))
        big, moved = b.relocate(pl)
        assert np.array_equal(kswlib.ref_extend_batch(P, big, moved[sel]), kswlib.ref_extend_batch(P, b.pool, b.tasks[sel]))
        b = batches["glb"]
        sel = np.nonzero(b.fam != bp.ORD)[0].tolist() + list(range(0, len(b.tasks), 7))
        big, moved = b.relocate(pl)
        r1, c1 = kswlib.ref_global_batch(P, big, moved[sel])
        r0, c0 = kswlib.ref_global_batch(P, b.pool, b.tasks[sel])
        assert np.array_equal(r1, r0) and all(np.array_equal(x, y) for x, y in zip(c1, c0))
        b = batches["sw"]
        big, moved = b.relocate(pl)
        got, want = kswlib.ref_sw_batch_mt(P, big, moved, 4), kswlib.ref_sw_batch_mt(P, b.pool, b.tasks, 4)
        for f in kswlib.SW_FIELDS:
            assert np.array_equal(got[f], want[f]), f"{pl}: ksw_align2 on the large pool differs in {f}"
