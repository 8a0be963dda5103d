"""The long-query Smith-Waterman kernel (csrc/sw_long.hip, bmh_ctx_set_wide_sw) against the compiled reference: mate-rescue
shaped word-mode tasks past qlen*max(mat) >= 32000 -- mates of 8-12 kb at -A 4 with true scores past 32 767, QREV|QCOMP mates,
BMH_F_TPAC windows on a resident pac -- bit-exact field for field; in-range long tasks identical with the switch on and off; a
mixed batch whose byte-mode mates keep their kernels; the LDS and slab variants; the *_device and *_sharded entry points; and a
context with the switch off still refusing.  Reference work stays near 10^10 cells on 16 threads."""
import numpy as np
import pytest

import devcalls
import kswgen
import kswlib
import swsatlib
import widesw as ws
from __graft_entry__ import load_package

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not kswlib.have_ref(), reason="oracle/_ref not built (no reference sources here)")]


def _ctx(p, wide=True):
    pkg = load_package()
    ctx = pkg.Context(0, p)
    if wide:
        ctx.set_wide_sw(True)
    return pkg, ctx


def _eq(got, want, tasks, what=""):
    devcalls.assert_sw(got, want, tasks, what)


def _ref(p, pool, tasks):
    return kswlib.ref_sw_batch_mt(p, pool, tasks, nthreads=16)


def test_long_mates_past_the_score_range_match_reference():
    rng = np.random.default_rng(9401)
    p = kswlib.make_params(a=4)
    specs = [(int(rng.integers(8000, 12001)), k % 4 != 3) for k in range(10)]
    pool, tasks = ws.gen_rescue(rng, p, specs, flank=1000)
    assert all(ws.goes_long(p, int(t["qlen"])) for t in tasks)
    pkg, ctx = _ctx(p)
    n0 = ctx.sw_wide_stats()[0]
    got = ctx.sw_batch(pool, tasks)
    assert ctx.sw_wide_stats()[0] - n0 == len(tasks) == ws.long_count(p, tasks)
    want = _ref(p, pool, tasks)
    _eq(got, want, tasks, "-A 4 long mates: ")
    assert (want["score"] == swsatlib.SAT).sum() >= 3, "saturation must be on the path"
    assert (want["tb"] >= 0).sum() >= 3 and (tasks["flags"] & kswlib.BMH_F_QCOMP).any()
    # the *_device and *_sharded entry points give the host call's records
    sw = devcalls.Sw(pool, tasks)
    sw.run(ctx)
    ctx.sync()
    _eq(sw.result(), got, tasks, "bmh_sw_batch_device: ")
    ctx2 = pkg.Context(0, p)
    ctx2.set_wide_sw(True)
    _eq(pkg.sw_batch_sharded([ctx, ctx2], pool, tasks), got, tasks, "bmh_sw_batch_sharded: ")
    ctx2.close()
    ctx.close()


def test_saturating_short_mates_and_tandem_ties():
    """-A 60..127 on 300-700 bp: the clamp on most diagonals, ties for qe, the second pass stopping at the first clamped row."""
    rng = np.random.default_rng(9402)
    for a, b in ((60, 90), (127, 127)):
        p = kswlib.make_params(a=a, b=b, o_del=6 * a // 4, e_del=a // 4, o_ins=5 * a // 4, e_ins=a // 3)
        pool, tasks = ws.concat(ws.gen_saturating(rng, p, 24), ws.gen_tandem(rng, p, 8))
        pkg, ctx = _ctx(p)
        got = ctx.sw_batch(pool, tasks)
        want = _ref(p, pool, tasks)
        _eq(got, want, tasks, f"-A {a}: ")
        assert (want["score"] == swsatlib.SAT).sum() >= 10
        ctx.close()


def test_tpac_windows_on_resident_pac():
    rng = np.random.default_rng(9403)
    p = kswlib.make_params(a=4)
    pool, tasks, pac, l_pac = ws.gen_rescue_tpac(rng, p, 400_000, [(8500, False), (9000, True), (8200, True), (3000, False)],
                                                 flank=800)
    pkg, ctx = _ctx(p)
    ctx.set_pac(pac, l_pac)
    n0 = ctx.sw_wide_stats()[0]
    got = ctx.sw_batch(pool, tasks)
    assert ctx.sw_wide_stats()[0] - n0 == len(tasks)
    want = kswlib.ref_sw_batch(p, pool, tasks, pac=pac, l_pac=l_pac)
    _eq(got, want, tasks, "TPAC: ")
    assert (want["score"] == swsatlib.SAT).sum() >= 2
    ctx.close()


def test_in_range_long_tasks_identical_switch_on_and_off():
    """1-5 kb at -A 1: the switch moves them from sw_generic_kernel to the new kernel (LDS variant up to 4 096 columns, slab
    variant past it) and nothing else changes."""
    rng = np.random.default_rng(9404)
    p = kswlib.make_params(a=1)
    specs = [(int(rng.integers(1000, 5001)), k % 5 != 4) for k in range(24)] + [(4097, True), (4600, True)]
    pool, tasks = ws.gen_rescue(rng, p, specs, flank=600, sub=0.03)
    assert (tasks["qlen"] > ws.LDS_COLS).sum() >= 3 and (tasks["qlen"] <= ws.LDS_COLS).sum() >= 10
    pkg, off = _ctx(p, wide=False)
    base = off.sw_batch(pool, tasks)
    assert off.sw_wide_stats()[0] == 0
    _, on = _ctx(p)
    got = on.sw_batch(pool, tasks)
    assert on.sw_wide_stats()[0] == len(tasks)
    _eq(got, base, tasks, "switch on vs off: ")
    orc, _ = kswlib.orc_sw_batch(p, pool, tasks, nthreads=16)
    _eq(got, orc, tasks, "oracle: ")
    off.close(), on.close()


def test_mixed_batch_keeps_short_mates_on_their_kernels():
    """150 bp byte-mode mates beside long word-mode ones (-A 1): the short ones keep their kernels and are not counted."""
    rng = np.random.default_rng(9405)
    p = kswlib.make_params(a=1)
    short = kswgen.gen_sw_materescue(rng, 300, p)
    longb = ws.gen_rescue(rng, p, [(int(rng.integers(6000, 9001)), True) for _ in range(3)] + [(2000, True)], flank=500)
    pool, tasks = ws.concat(short, longb)
    tasks = tasks[rng.permutation(len(tasks))]
    is_long = tasks["qlen"] >= 2000
    assert (tasks["xtra"][~is_long] & kswlib.KSW_XBYTE).all()
    pkg, on = _ctx(p)
    got = on.sw_batch(pool, tasks)
    assert on.sw_wide_stats()[0] == ws.long_count(p, tasks) == int(is_long.sum())
    _, off = _ctx(p, wide=False)
    _eq(got, off.sw_batch(pool, tasks), tasks, "switch on vs off: ")
    _eq(got, _ref(p, pool, tasks), tasks, "mixed batch: ")
    off.close(), on.close()


def test_small_batch_branch_reaches_the_new_kernel():
    """A batch small enough for one wave per task (sw_wave_fits): its word-mode tasks with scores of 512 and more, which
    sw_wave_kernel leaves, reach the new kernel too; so does a batch of one long task."""
    rng = np.random.default_rng(9407)
    p = kswlib.make_params(a=4)
    pool, tasks = kswgen.gen_sw_materescue(rng, 50, p, read_len=(200, 300))
    assert not (tasks["xtra"] & kswlib.KSW_XBYTE).any()
    pkg, on = _ctx(p)
    _, off = _ctx(p, wide=False)
    got = on.sw_batch(pool, tasks)
    assert on.sw_wide_stats()[0] == len(tasks)
    _eq(got, off.sw_batch(pool, tasks), tasks, "small batch, switch on vs off: ")
    _eq(got, _ref(p, pool, tasks), tasks, "small batch: ")
    lpool, one = ws.gen_rescue(rng, p, [(9000, True)], flank=400)
    _eq(on.sw_batch(lpool, one), _ref(p, lpool, one), one, "single long task: ")
    assert on.sw_wide_stats()[0] == len(tasks) + 1
    off.close(), on.close()


def test_switch_off_still_refuses_and_stays_exact():
    rng = np.random.default_rng(9406)
    p = kswlib.make_params(a=4)
    pool, tasks = ws.gen_rescue(rng, p, [(8100, True)], flank=300)
    pkg, ctx = _ctx(p, wide=False)
    with pytest.raises(pkg.BmhError) as e:
        ctx.sw_batch(pool, tasks)
    assert e.value.code == pkg.BMH_E_RANGE
    spool, st = kswgen.gen_sw_materescue(rng, 64, p)
    want, _ = kswlib.orc_sw_batch(p, spool, st)
    _eq(ctx.sw_batch(spool, st), want, st, "after a refusal: ")
    ctx.set_wide_sw(True)
    _eq(ctx.sw_batch(pool, tasks), _ref(p, pool, tasks), tasks, "switched on: ")
    ctx.set_wide_sw(False)
    with pytest.raises(pkg.BmhError):
        ctx.sw_batch(pool, tasks)
    ctx.close()
