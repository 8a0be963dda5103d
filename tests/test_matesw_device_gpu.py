"""Mate rescue on the device: bmh_matesw_device == the committed fixture (the compiled reference's own loop), == the oracle's
orc_matesw_pair and == bmh_matesw_batch on the generated batches of tests/mswgen.py -- multi-round pairs, vectors grown from nothing to a
dozen regions, regions for mem_sort_and_dedup to remove, anchors at the strand ends, word mode -- which is also the first time the host
driver meets such inputs.  Then shapes (active pairs among inactive ones, nothing to do, a second batch on the same context) and the
refusals, each of which must leave the caller's vectors as they were."""
import numpy as np
import pytest

import kswlib
import mswgen
from __graft_entry__ import load_package
from test_kernel_families_gpu import _ctx_with

pytestmark = pytest.mark.gpu

STATS = ("rounds", "ext_tasks", "pool_bytes")


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


def _device(ctx, sc, table, opt, reads, regs):
    ctx.set_params(mswgen.scoring(sc))
    got, ns = ctx.matesw_device(mswgen.L_PAC, reads, regs, mswgen.pes(table), mswgen.opt(opt), mswgen.LEVEL)
    return got, ns, ctx.driver_stats()


def _host(ctx, sc, table, opt, reads, regs):
    ctx.set_params(mswgen.scoring(sc))
    got, ns = ctx.matesw_batch(mswgen.L_PAC, ctx._msw_pac, reads, regs, mswgen.pes(table), mswgen.opt(opt), mswgen.bmh_dedup_callback(mswgen.LEVEL))
    return got, ns, ctx.driver_stats()


def test_fixture_all_groups():
    """the six groups of matesw_golden.npz at their own mask_level_redun"""
    c = _ctx_with({})
    g = kswlib.load_golden("matesw_golden.npz")
    calls = 0
    for key, (p, o, pes, l_pac, pac, reads, regs, exp, n_sw) in zip(g["groups"], kswlib.golden_matesw_groups()):
        c.set_params(p)
        c.set_pac(pac, l_pac)
        got, ns = c.matesw_device(l_pac, reads, regs, pes, o, float(g[str(key) + "mask_level_redun"]))
        assert ns == n_sw
        _same(got, exp, str(key))
        calls += sum(ns)
    assert calls > 4000
    c.close()


@pytest.mark.parametrize("sc", ["byte", "word"])
@pytest.mark.parametrize("opt", list(mswgen.OPTS))
@pytest.mark.parametrize("table", ["fr", "all"])
def test_generated_batches_match_oracle_and_host_driver(ctx, table, opt, sc):
    reads, regs = mswgen.main_batch(sc)
    want, wn, removed = mswgen.oracle("main", sc, table, opt)
    if opt == "default":  # the ground the batch is made to reach, on the oracle's side
        if table == "fr":
            assert sum(n > 8 for n in wn) >= 40  # more than LOOKAHEAD invocations: a second round
        else:
            assert max(len(w) for w, r in zip(want, regs) if len(r) == 0) >= 10 and removed >= 10
    got, gn, gst = _device(ctx, sc, table, opt, reads, regs)
    host, hn, hst = _host(ctx, sc, table, opt, reads, regs)
    print(table, opt, sc, "device", {k: gst[k] for k in STATS}, "host", {k: hst[k] for k in STATS}, "calls", sum(wn))
    assert gn == wn
    _same(got, want, "device against the oracle")
    assert hn == wn
    _same(host, want, "host driver against the oracle")
    assert {k: gst[k] for k in STATS} == {k: hst[k] for k in STATS}
    if table == "fr" and opt == "default":
        assert gst["rounds"] >= 2


@pytest.mark.parametrize("shape", [(1, 9), (65, 40), (130, 60)])
def test_active_pairs_among_inactive_ones(ctx, shape):
    reads, regs = mswgen.mixed_batch(*shape)
    want, wn, _ = mswgen.oracle(shape, "byte", "fr", "default")
    got, gn, st = _device(ctx, "byte", "fr", "default", reads, regs)
    assert gn == wn and sum(n > 0 for n in wn) >= shape[0] * 3 // 4
    _same(got, want, str(shape))
    assert st["pool_bytes"] < sum(len(r) for r in reads)  # the inactive pairs' reads stay on the host


def test_nothing_to_do_answers_ok(ctx):
    reads, regs = mswgen.mixed_batch(0, 30)
    got, gn, st = _device(ctx, "byte", "fr", "default", reads, regs)
    _same(got, regs, "all inactive")
    assert gn == [0] * 30 and st["rounds"] == 0 and st["ext_tasks"] == 0
    got, gn, _ = _device(ctx, "byte", "fr", "default", [], [])
    assert got == [] and gn == []
    reads, regs = mswgen.main_batch("byte")
    got, gn, st = _device(ctx, "byte", "none", "default", reads, regs)  # all four orientations failed
    _same(got, regs, "all failed")
    assert gn == [0] * (len(reads) // 2) and st["rounds"] == 0


def test_second_batch_on_the_same_context():
    """small, large, small again on a fresh context: workspace regrowth and nothing stale"""
    c = _ctx_with({})
    l_pac, pac, _ = mswgen.genome()
    c._msw_pac = c.set_pac(pac, l_pac)
    for batch in ((1, 9), "main", (65, 40), (1, 9)):
        reads, regs = mswgen.main_batch("byte") if batch == "main" else mswgen.mixed_batch(*batch)
        want, wn, _ = mswgen.oracle(batch, "byte", "fr" if batch != "main" else "all", "default")
        got, gn, _ = _device(c, "byte", "fr" if batch != "main" else "all", "default", reads, regs)
        assert gn == wn
        _same(got, want, str(batch))
    c.close()


def _refused(c, code, reads, regs, table="fr", sc="byte"):
    pkg = load_package()
    with pytest.raises(pkg.BmhError) as e:
        _device(c, sc, table, "default", reads, regs)
    assert e.value.code == code, e.value
    _same(e.value.regs, regs, "a refused call")


def _good_call(c):
    reads, regs = mswgen.mixed_batch(1, 9)
    want, wn, _ = mswgen.oracle((1, 9), "byte", "fr", "default")
    got, gn, _ = _device(c, "byte", "fr", "default", reads, regs)
    assert gn == wn
    _same(got, want, "a good call after a refusal")


def test_refusals_leave_the_vectors_untouched():
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
        c.matesw_device(l_pac - 4, reads, regs, mswgen.pes("fr"), mswgen.opt("default"), mswgen.LEVEL)
    assert e.value.code == pkg.BMH_E_ARG
    _same(e.value.regs, regs, "another l_pac")
    # an active pair with a read of 0 bases, and one with a read of 65 536 bases
    for n_bases in (0, 65536):
        bad = list(reads)
        bad[2 * active + 1] = np.random.default_rng(3).integers(0, 4, n_bases).astype(np.uint8)
        _refused(c, pkg.BMH_E_RANGE, bad, regs)
        _good_call(c)
    # the same lengths in a pair that needs no rescue are nobody's business
    idle = next(p for p, n in enumerate(wn) if n == 0)
    odd = list(reads)
    odd[2 * idle] = np.zeros(0, np.uint8)
    got, gn, _ = _device(c, "byte", "fr", "default", odd, regs)
    assert gn == wn
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
        c.matesw_device(l_pac, reads, regs, *args, mswgen.LEVEL)
    assert e.value.code == pkg.BMH_E_RANGE
    _same(e.value.regs, regs, "past the 16-bit range")
    _good_call(c)
    c.set_params(p)
    c.set_wide_sw(True)
    got, gn = c.matesw_device(l_pac, reads, regs, *args, mswgen.LEVEL)
    gst = c.driver_stats()
    host, hn = c.matesw_batch(l_pac, c._msw_pac, reads, regs, *args, mswgen.bmh_dedup_callback(mswgen.LEVEL))
    hst = c.driver_stats()
    assert gn == hn and gn[0] == 1 and len(got[1]) == 1  # the mate is found
    _same(got, host, "under the wide switch")
    assert {k: gst[k] for k in STATS} == {k: hst[k] for k in STATS}
    c.close()
