"""Pairing and mate rescue on the device with all four orientations open (tests/golden/orient_golden.npz, tests/orientgen.py; the CPU
side is tests/test_orient_cpu.py).  Under the FR-only tables of every other test bmh_decide_device's pair table
term[term_off[dir] + dist - pes[dir].low] has had the offsets {0, 0, 0, 0}, and msw_round_kernel has never rescued a mate that is not
reverse-complemented or lies upstream.  Here:
 * decide_device == decide_batch byte for byte and == the reference's mem_pair on every pairing group, at 1, 64, 65 and 400 pairs and
   at an id where mem_pair's `(int)id << 8` truncates;
 * the pair table's accounting: four windows that fit singly but not together are refused, four that just fit are decided;
 * matesw_batch (host driver over the SW kernels) and matesw_device == the reference's own rescue on every rescue group, in byte and
   word mode, and equal to each other down to rounds, tasks and pool bytes; a batch of active pairs among inactive ones == the oracle."""
import numpy as np
import pytest

import decidegen as dg
import kswgen
import kswlib
import mswgen
import orientgen as og
from __graft_entry__ import load_package
from test_decide_device_gpu import E_RANGE, _sam_batch
from test_kernel_families_gpu import _ctx_with
from test_matesw_device_gpu import STATS, _same

pytestmark = pytest.mark.gpu

PAIR_KEYS = [f"p{si}_{mix}_" for si in (0, 2) for mix in og.MIXES]
RESCUE_KEYS = ["rbytev0_", "rbytev1_", "rwordv0_", "rwordv1_"]
ID0 = 2000  # pair p under id 1000 + p, the fixture's


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0, kswlib.make_params())
    yield c
    c.close()


def _both(pkg, ctx, o, l_pac, pes, id0, vecs, what):
    host = pkg.decide_batch(o, l_pac, pes, id0, vecs)
    dev = ctx.decide_device(o, l_pac, pes, id0, vecs)
    dg.assert_same(dev, host, what)
    assert ctx.last_decide_stats()[:2] == (len(vecs) // 2, 0), what
    return dev


def _offsets_in_play(pes):
    """term_off[1] > 0: orientation 0 is open with a window that is not empty"""
    return not int(pes[0]["failed"]) and int(pes[0]["high"]) >= int(pes[0]["low"])


# ---------------------------------------------------------------- decisions

@pytest.mark.parametrize("key", PAIR_KEYS)
def test_decide_device_on_the_pairing_groups(pkg, ctx, key):
    _, si, mix, l_pac, vecs, _, pes, pr = og.pairing_group(key)
    if mix == "all4":
        assert _offsets_in_play(pes) and (pes["failed"] == 0).all()
    dev = _both(pkg, ctx, dg.pe_opt(si), l_pac, pes, ID0, vecs, key)
    pd = dev["pd"]
    assert (pd["score"] == pr[:, 0]).all() and (pd["sub"] == pr[:, 1]).all() and (pd["n_sub"] == pr[:, 2]).all()
    pair_won = (pd["paired"] != 0) & ((pd["extra_flag"] & 2) != 0)
    assert pair_won.sum() > 50
    assert (pd["z"][pair_won] == og.marked_pair_res(key)[pair_won, 3:5]).all()  # (z indexes the marked vectors)


@pytest.mark.parametrize("units", [1, 64, 65, 400])
def test_unit_counts_with_four_open_orientations(pkg, ctx, units):
    for key in ("p0_all4_", "p2_all4_"):
        _, si, _, l_pac, vecs, _, pes, pr = og.pairing_group(key)
        assert _offsets_in_play(pes)
        dev = _both(pkg, ctx, dg.pe_opt(si), l_pac, pes, ID0, vecs[:2 * units], f"{key} {units} pairs")
        assert (dev["pd"]["score"] == pr[:units, 0]).all() and (dev["pd"]["n_sub"] == pr[:units, 2]).all()


def test_truncating_id_with_four_open_orientations(pkg, ctx):
    _, si, _, l_pac, vecs, _, pes, _ = og.pairing_group("p0_all4_")
    assert _offsets_in_play(pes)
    dev = _both(pkg, ctx, dg.pe_opt(si), l_pac, pes, dg.ID0_TRUNCATING[1], vecs, "truncating id0")
    assert dev["pd"]["paired"].sum() > 100


# ---------------------------------------------------------------- the pair table's accounting

def _wide_tables():
    """(four windows of 2^18 + 1 distances, four of exactly 2^18): either fits the table of 2^20 entries alone, four of the first
    do not; the lows differ, so that every orientation's offset and low matter"""
    _, _, _, _, _, _, pes, _ = og.pairing_group("p0_all4_")
    over, fits = pes.copy(), pes.copy()
    for d in range(4):
        over[d]["low"] = fits[d]["low"] = 1 + 4 * d
        over[d]["high"] = int(over[d]["low"]) + (1 << 18)
        fits[d]["high"] = int(fits[d]["low"]) + (1 << 18) - 1
    assert all(int(t["high"][d]) - int(t["low"][d]) + 1 <= 1 << 20 for t in (over, fits) for d in range(4))
    assert sum(int(over["high"][d]) - int(over["low"][d]) + 1 for d in range(4)) == (1 << 20) + 4
    assert sum(int(fits["high"][d]) - int(fits["low"][d]) + 1 for d in range(4)) == 1 << 20
    return over, fits


def test_pair_table_is_accounted_over_all_four_windows(pkg, ctx):
    _, si, _, l_pac, vecs, _, _, _ = og.pairing_group("p0_all4_")
    o = dg.pe_opt(si)
    over, fits = _wide_tables()
    vecs = [np.ascontiguousarray(v) for v in vecs[:80]]
    before = [v.tobytes() for v in vecs]
    with pytest.raises(pkg.BmhError) as e:
        ctx.decide_device(o, l_pac, over, ID0, vecs, inplace=True)
    assert e.value.code == E_RANGE
    assert [v.tobytes() for v in vecs] == before
    assert ctx.last_decide_stats()[:2] == (0, 1)
    dev = _both(pkg, ctx, o, l_pac, fits, ID0, vecs, "four windows of 2^18")
    assert [v.tobytes() for v in vecs] == before  # (not in place)
    assert (dev["pd"]["score"] > 0).sum() >= 20  # windows this wide pair most of the 40


def test_refused_pair_table_falls_back_behind_sam_batch(pkg, ctx):
    _, si, _, l_pac, vecs, _, _, _ = og.pairing_group("p0_all4_")
    assert l_pac == dg.L_PAC
    o = dg.pe_opt(si)
    over, fits = _wide_tables()
    vecs = vecs[:120]
    rng = np.random.default_rng(41)
    ref = kswgen.rand_seq(rng, l_pac)
    reads = [kswgen.rand_seq(rng, 150) for _ in vecs]
    try:
        for pes, stats in ((over, (0, 1)), (fits, (len(vecs) // 2, 0))):
            ctx.set_decide_device(False)
            t0, r0 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, ref, reads)
            ctx.set_decide_device(True)
            t1, r1 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, ref, reads)
            assert t0 == t1 and r0 == r1
            assert ctx.last_decide_stats()[:2] == stats
            assert sum(len(t.splitlines()) for t in t0) >= len(vecs)
    finally:
        ctx.set_decide_device(False)


# ---------------------------------------------------------------- mate rescue

@pytest.fixture(scope="module")
def msw_ctx():
    c = _ctx_with({})
    g = og.golden()
    c._orient_pac = c.set_pac(g["pac"], int(g["l_pac"]))
    yield c
    c.close()


@pytest.mark.parametrize("key", RESCUE_KEYS)
def test_rescue_groups_on_host_driver_and_device(msw_ctx, key):
    c = msw_ctx
    _, p, o, pes, l_pac, pac, reads, regs, orient, exp, n_sw, level = next(x for x in og.rescue_groups() if x[0] == key)
    assert (pes["failed"] == 0).all()
    c.set_params(p)
    got, gn = c.matesw_device(l_pac, reads, regs, pes, o, level)
    gst = c.driver_stats()
    host, hn = c.matesw_batch(l_pac, c._orient_pac, reads, regs, pes, o, mswgen.bmh_dedup_callback(level))
    hst = c.driver_stats()
    print(key, "device", {k: gst[k] for k in STATS}, "host", {k: hst[k] for k in STATS}, "calls", sum(n_sw))
    assert gn == n_sw
    _same(got, exp, key + " device against the reference")
    assert hn == n_sw
    _same(host, exp, key + " host driver against the reference")
    assert {k: gst[k] for k in STATS} == {k: hst[k] for k in STATS}
    assert sum(n_sw) > 1500 and gst["rounds"] >= 1


def test_four_orientation_pairs_among_inactive_ones(msw_ctx):
    """65 pairs that need rescue (16 or 17 of each orientation) among 40 that need none -- with all four orientations open those are
    the pairs without any hit -- in one batch, against the oracle"""
    c = msw_ctx
    _, p, o, pes, l_pac, pac, reads, regs, orient, _, n_sw, level = next(x for x in og.rescue_groups() if x[0] == "rbytev0_")
    n_sw = np.array(n_sw)
    active = np.concatenate([np.nonzero((n_sw > 0) & (orient == d))[0][:17 if d == 0 else 16] for d in range(4)])
    assert len(active) == 65
    rng = np.random.default_rng(8)
    pick = rng.permutation(np.concatenate([active, np.full(40, -1)]))
    b_reads = [reads[2 * k + r] if k >= 0 else kswgen.rand_seq(rng, 130) for k in pick for r in range(2)]
    b_regs = [regs[2 * k + r] if k >= 0 else regs[0][:0] for k in pick for r in range(2)]
    want, wn = kswlib.orc_matesw_pairs(p, o, l_pac, pac, pes, b_reads, b_regs, mswgen.bmh_dedup_callback(level))
    assert wn == [int(n_sw[k]) if k >= 0 else 0 for k in pick]
    c.set_params(p)
    got, gn = c.matesw_device(l_pac, b_reads, b_regs, pes, o, level)
    assert gn == wn
    _same(got, want, "device against the oracle")
    assert c.driver_stats()["pool_bytes"] < sum(len(r) for r in b_reads)  # the inactive pairs' reads stay on the host
    host, hn = c.matesw_batch(l_pac, c._orient_pac, b_reads, b_regs, pes, o, mswgen.bmh_dedup_callback(level))
    assert hn == wn
    _same(host, want, "host driver against the oracle")
