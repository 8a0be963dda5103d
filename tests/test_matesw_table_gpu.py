"""Mate rescue over a flat region table: bmh_matesw_table_device == the committed fixture (the compiled reference's own loop), == the
oracle and == bmh_matesw_device on the generated batches of tests/mswgen.py, with the same rounds and ksw_align2 calls.  Then shapes
(active pairs among inactive ones across a wave and across a scan block, nothing to do, contexts that are used again and shared with
bmh_matesw_device), what crosses PCIe between the upload and the download, and the refusals, each of which must leave the outputs as
they were."""
import numpy as np
import pytest

import kswlib
import mswgen
import orientgen as og
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

STATS = ("rounds", "ext_tasks")
PLAN_BYTES, STATUS_BYTES, TOTAL_BYTES = 64, 16, 16
SCAN_BLOCK = 256  # kMtScanThreads, csrc/matesw.hip


def _same(got, exp, what):
    assert len(got) == len(exp)
    for k, (a, b) in enumerate(zip(got, exp)):
        assert len(a) == len(b) and a.tobytes() == b.tobytes(), f"{what}: vector {k} (pair {k // 2}): got {a}, want {b}"


@pytest.fixture(scope="module")
def ctx():
    c = _ctx_with({})
    l_pac, pac, _ = mswgen.genome()
    c._msw_pac = c.set_pac(pac, l_pac)
    yield c
    c.close()


def _table(ctx, sc, table, opt, reads, regs, **kw):
    ctx.set_params(mswgen.scoring(sc))
    got, ns = ctx.matesw_table_device(mswgen.L_PAC, reads, regs, mswgen.pes(table), mswgen.opt(opt), mswgen.LEVEL, **kw)
    st, mt = ctx.driver_stats(), ctx.last_matesw_table_stats()
    _stats_hold(mt, st, reads, regs, got)
    return got, ns, st, mt


def _device(ctx, sc, table, opt, reads, regs):
    ctx.set_params(mswgen.scoring(sc))
    got, ns = ctx.matesw_device(mswgen.L_PAC, reads, regs, mswgen.pes(table), mswgen.opt(opt), mswgen.LEVEL)
    return got, ns, ctx.driver_stats()


def _stats_hold(mt, st, reads, regs, got):
    """what every successful call's statistics must say"""
    print("table stats", mt, "driver", {k: st[k] for k in STATS + ("pool_bytes",)})
    assert mt["pairs"] == len(reads) // 2 and mt["regions_in"] == sum(len(r) for r in regs) and mt["regions_out"] == sum(len(r) for r in got)
    backs = mt["waits"] - 2  # status read-backs: one per round kernel
    assert mt["mid_bytes"] == PLAN_BYTES + STATUS_BYTES * backs + TOTAL_BYTES  # no region, no read and no count crossed in between
    assert (backs == 0) == (mt["active"] == 0) and backs >= st["rounds"]
    assert st["pool_bytes"] == (sum(len(r) for r in reads) + 16 if st["rounds"] else 0)
    assert (mt["arena_records"] == 0) == (mt["active"] == 0) and mt["hits"] <= mt["arena_records"]
    assert mt["filter_ms"] == mt["pack_ms"] == mt["merge_ms"] == -1.0  # kernel timing is off


def test_fixture_all_groups():
    """the six groups of matesw_golden.npz at their own mask_level_redun"""
    c = _ctx_with({})
    g = kswlib.load_golden("matesw_golden.npz")
    calls = 0
    for key, (p, o, pes, l_pac, pac, reads, regs, exp, n_sw) in zip(g["groups"], kswlib.golden_matesw_groups()):
        c.set_params(p)
        c.set_pac(pac, l_pac)
        got, ns = c.matesw_table_device(l_pac, reads, regs, pes, o, float(g[str(key) + "mask_level_redun"]))
        assert ns == n_sw
        _same(got, exp, str(key))
        calls += sum(ns)
    assert calls > 4000
    c.close()


@pytest.mark.parametrize("sc", ["byte", "word"])
@pytest.mark.parametrize("opt", list(mswgen.OPTS))
@pytest.mark.parametrize("table", ["fr", "all"])
def test_generated_batches_match_oracle_and_device_driver(ctx, table, opt, sc):
    reads, regs = mswgen.main_batch(sc)
    want, wn, _ = mswgen.oracle("main", sc, table, opt)
    got, gn, gst, mt = _table(ctx, sc, table, opt, reads, regs)
    dev, dn, dst = _device(ctx, sc, table, opt, reads, regs)
    assert gn == wn
    _same(got, want, "table against the oracle")
    assert dn == wn
    _same(dev, want, "device driver against the oracle")
    assert {k: gst[k] for k in STATS} == {k: dst[k] for k in STATS}
    if table == "fr" and opt == "default":
        assert gst["rounds"] >= 2


@pytest.mark.parametrize("shape", [(1, 9), (65, 40), (130, 60)])
def test_active_pairs_among_inactive_ones(ctx, shape):
    reads, regs = mswgen.mixed_batch(*shape)
    want, wn, _ = mswgen.oracle(shape, "byte", "fr", "default")
    got, gn, st, mt = _table(ctx, "byte", "fr", "default", reads, regs)
    assert gn == wn
    _same(got, want, str(shape))
    assert mt["active"] >= shape[0] * 3 // 4 and 0 < mt["active"] < mt["pairs"]


def test_more_pairs_than_a_scan_block(ctx):
    """348 pairs: two blocks of the pairs' scan, three of the vectors', with active pairs in both"""
    reads, regs = mswgen.mixed_batch(48, 300)
    dev, dn, dst = _device(ctx, "byte", "fr", "default", reads, regs)
    rescued = [p for p, n in enumerate(dn) if n > 0]
    assert len(reads) // 2 > SCAN_BLOCK and sum(p < SCAN_BLOCK for p in rescued) >= 3 and sum(p >= SCAN_BLOCK for p in rescued) >= 3
    got, gn, gst, mt = _table(ctx, "byte", "fr", "default", reads, regs)
    assert gn == dn
    _same(got, dev, "table against the device driver")
    assert {k: gst[k] for k in STATS} == {k: dst[k] for k in STATS}
    assert mt["active"] >= 48 * 3 // 4 and 0 < mt["active"] < mt["pairs"]


def test_nothing_to_do_copies_the_table(ctx):
    for reads, regs, table in (mswgen.mixed_batch(0, 30) + ("fr",), ([], [], "fr"), mswgen.main_batch("byte") + ("none",)):
        got, gn, st, mt = _table(ctx, "byte", table, "default", reads, regs)
        _same(got, regs, "nothing to do under " + table)
        assert gn == [0] * (len(reads) // 2) and st["rounds"] == 0 and st["ext_tasks"] == 0 and mt["active"] == 0
        assert mt["mid_bytes"] == PLAN_BYTES + TOTAL_BYTES and mt["waits"] == 2


def test_host_traffic_between_upload_and_download(ctx):
    """plan + 16 bytes per status read-back + total: 105 pairs' regions, reads and counts stay on the device"""
    reads, regs = mswgen.mixed_batch(65, 40)
    got, gn, st, mt = _table(ctx, "byte", "fr", "default", reads, regs)
    backs = mt["waits"] - 2
    assert backs >= 2 and st["rounds"] >= 1
    assert mt["mid_bytes"] == PLAN_BYTES + STATUS_BYTES * backs + TOTAL_BYTES < 64 * 16  # less than sixteen regions' bytes
    assert mt["regions_out"] > mt["regions_in"] > 65


def test_contexts_are_used_again_and_shared_with_the_device_driver():
    """small, large, small again on a fresh context, bmh_matesw_device in between: both drivers' blocks lie in the same buffer"""
    c = _ctx_with({})
    l_pac, pac, _ = mswgen.genome()
    c._msw_pac = c.set_pac(pac, l_pac)
    for batch, call in (((1, 9), _table), ("main", _table), ((65, 40), _device), ((1, 9), _table), ("main", _device), ((65, 40), _table)):
        reads, regs = mswgen.main_batch("byte") if batch == "main" else mswgen.mixed_batch(*batch)
        table = "fr" if batch != "main" else "all"
        want, wn, _ = mswgen.oracle(batch, "byte", table, "default")
        got, gn = call(c, "byte", table, "default", reads, regs)[:2]
        assert gn == wn
        _same(got, want, str(batch))
    c.close()


def _refused(c, code, reads, regs, table="fr", sc="byte", **kw):
    pkg = load_package()
    with pytest.raises(pkg.BmhError) as e:
        _table(c, sc, table, "default", reads, regs, **kw)
    assert e.value.code == code, e.value
    roff_out, reg_ptr, n_sw = e.value.outputs
    assert (roff_out == 0xdeadbeefdeadbeef).all() and reg_ptr is None and (n_sw == -77).all(), "a refused call wrote its outputs"
    return str(e.value)


def _good_call(c):
    reads, regs = mswgen.mixed_batch(1, 9)
    want, wn, _ = mswgen.oracle((1, 9), "byte", "fr", "default")
    got, gn, _, _ = _table(c, "byte", "fr", "default", reads, regs)
    assert gn == wn
    _same(got, want, "a good call after a refusal")


def test_refusals_leave_the_outputs_untouched():
    pkg = load_package()
    c = _ctx_with({})
    l_pac, pac, _ = mswgen.genome()
    reads, regs = mswgen.mixed_batch(1, 9)
    _, wn, _ = mswgen.oracle((1, 9), "byte", "fr", "default")
    active = next(p for p, n in enumerate(wn) if n > 0)
    # no resident reference
    _refused(c, pkg.BMH_E_ARG, reads, regs)
    c._msw_pac = c.set_pac(pac, l_pac)
    _good_call(c)
    # a reference of another l_pac
    with pytest.raises(pkg.BmhError) as e:
        c.matesw_table_device(l_pac - 4, reads, regs, mswgen.pes("fr"), mswgen.opt("default"), mswgen.LEVEL)
    assert e.value.code == pkg.BMH_E_ARG and (e.value.outputs[0] == 0xdeadbeefdeadbeef).all() and e.value.outputs[1] is None
    # an active pair with a read of 0 bases, and one with a read of 65 536 bases: the plan record names the read
    for n_bases in (0, 65536):
        bad = list(reads)
        bad[2 * active + 1] = np.random.default_rng(3).integers(0, 4, n_bases).astype(np.uint8)
        text = _refused(c, pkg.BMH_E_RANGE, bad, regs)
        assert f"read {2 * active + 1} of a pair that needs rescue has {n_bases} bases (1..65535)" in text, text
        _good_call(c)
    # the same lengths in a pair that needs no rescue are nobody's business
    idle = next(p for p, n in enumerate(wn) if n == 0)
    for n_bases in (0, 65536):
        odd = list(reads)
        odd[2 * idle] = np.zeros(n_bases, np.uint8)
        got, gn, _, _ = _table(c, "byte", "fr", "default", odd, regs)
        assert gn == wn
    # offsets that run backwards
    roff = np.concatenate([[0], np.cumsum([len(v) for v in regs])]).astype(np.uint64)
    k = next(k for k in range(len(regs)) if roff[k] > 0)
    back = roff.copy()
    back[k + 1] = back[k] - 1
    _refused(c, pkg.BMH_E_ARG, reads, regs, roff=back)
    first = roff.copy()
    first[0] = 1
    _refused(c, pkg.BMH_E_ARG, reads, regs, roff=first)
    _good_call(c)
    c.close()


def test_word_mode_past_the_16_bit_range_needs_the_wide_switch():
    """l_seq * max(mat) >= 32000 (320 bases at a = 100): refused without bmh_ctx_set_wide_sw, accepted with it, and then what the host
    driver gives under the same switch"""
    pkg = load_package()
    c = _ctx_with({})
    l_pac, pac, ref = mswgen.genome()
    c._msw_pac = c.set_pac(pac, l_pac)
    p = kswlib.make_params(a=100, b=110, o_del=120, e_del=30, o_ins=120, e_ins=30)
    x = mswgen.FREE0 + 700
    reads = [ref[x: x + 320].copy(), mswgen.revcomp(ref[x + 330: x + 650])]
    regs = [mswgen._vector([mswgen._region(x, 320, 320, 100)]), mswgen._vector([])]
    reads2, regs2 = mswgen.mixed_batch(1, 9)
    reads, regs = reads + reads2, regs + regs2
    c.set_params(p)
    args = (mswgen.pes("fr"), mswgen.opt("default"))
    with pytest.raises(pkg.BmhError) as e:
        c.matesw_table_device(l_pac, reads, regs, *args, mswgen.LEVEL)
    assert e.value.code == pkg.BMH_E_RANGE and "read 0: l_seq*max(mat) reaches the 16-bit score range" in str(e.value)
    assert (e.value.outputs[0] == 0xdeadbeefdeadbeef).all() and e.value.outputs[1] is None and (e.value.outputs[2] == -77).all()
    _good_call(c)
    c.set_params(p)
    c.set_wide_sw(True)
    got, gn = c.matesw_table_device(l_pac, reads, regs, *args, mswgen.LEVEL)
    gst = c.driver_stats()
    host, hn = c.matesw_batch(l_pac, c._msw_pac, reads, regs, *args, mswgen.bmh_dedup_callback(mswgen.LEVEL))
    hst = c.driver_stats()
    assert gn == hn and gn[0] == 1 and len(got[1]) == 1  # the mate is found
    _same(got, host, "under the wide switch")
    assert {k: gst[k] for k in STATS} == {k: hst[k] for k in STATS}
    c.close()


def test_kernel_timing_reports_the_three_groups(ctx):
    reads, regs = mswgen.mixed_batch(65, 40)
    ctx.set_kernel_timing(True)
    try:
        ctx.set_params(mswgen.scoring("byte"))
        ctx.matesw_table_device(mswgen.L_PAC, reads, regs, mswgen.pes("fr"), mswgen.opt("default"), mswgen.LEVEL)
        mt = ctx.last_matesw_table_stats()
    finally:
        ctx.set_kernel_timing(False)
    print(mt)
    assert mt["filter_ms"] > 0 and mt["pack_ms"] > 0 and mt["merge_ms"] > 0


@pytest.mark.parametrize("d", range(4))
def test_one_batch_per_library_orientation(d):
    """the committed all-orientations rescue group, cut into one batch per orientation of its pairs"""
    c = _ctx_with({})
    _, p, o, pes, l_pac, pac, reads, regs, orient, _, n_sw, level = next(x for x in og.rescue_groups() if x[0] == "rbytev0_")
    c.set_pac(pac, l_pac)
    pick = np.nonzero(orient == d)[0][:40]
    assert len(pick) >= 20 and sum(n_sw[k] > 0 for k in pick) >= 10
    b_reads = [reads[2 * k + r] for k in pick for r in range(2)]
    b_regs = [regs[2 * k + r] for k in pick for r in range(2)]
    c.set_params(p)
    dev, dn = c.matesw_device(l_pac, b_reads, b_regs, pes, o, level)
    dst = c.driver_stats()
    got, gn = c.matesw_table_device(l_pac, b_reads, b_regs, pes, o, level)
    gst = c.driver_stats()
    assert gn == dn == [int(n_sw[k]) for k in pick]
    _same(got, dev, f"orientation {og.NAMES[d]}")
    assert {k: gst[k] for k in STATS} == {k: dst[k] for k in STATS} and gst["rounds"] >= 1
    c.close()
