"""bmh_pairs_sam_device: paired-end reads to SAM text with the region table on the device from the kernel that makes it, through mate
rescue, to the kernel that sorts it.  Against the compiled reference's SAM body for the fixture's two paired-end runs (tests/pipechain.py
over tests/golden/pipeline_golden.npz), against the composition it replaces (bmh_seed_chain_regs_batch with its three switches,
bmh_pestat_from_candidates or the caller's table, bmh_matesw_device, bmh_phase2_text_device) text for text and number for number,
and against what a quiet download or upload of the regions would break: the bytes between the phases do not grow with the regions,
phase 2 uploads at least 64 bytes per region less than the composition.  Then the block edges of table_plan_kernel with rescue live
and with a table of four failed orientations, batches with few or no regions, one mate of every pair unalignable, -e, one context
through the call and the other routes in turn, and the refusals."""
import ctypes as C
import types

import numpy as np
import pytest

import handoff_ref as hr
import pipechain as pc
from __graft_entry__ import load_package
from test_pairs_plan_core_cpu import pair_kmax
from test_pestat_cand_cpu import bits
from test_reads_sam_device_gpu import _exact_reads
from test_reads_sam_device_gpu import call as se_call

pytestmark = pytest.mark.gpu

PE = ("pe0", "pe1")
P2_KEYS = ("units", "wanted", "fixed", "redone", "reads", "lines", "text_bytes", "d2h_bytes", "fallbacks", "sessions", "waits")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _seqs(r):
    return [(r.names[i], None, r.reads[i], r.quals[i]) for i in range(len(r.reads))]


def call(c, r, id0=0, pes0=None, opt=None, smem=None, out=None):
    """the call on c, and what its statistics and the other calls' say afterwards"""
    c.set_params(r.params), c.set_region_long(True)
    text, off, pes = c.pairs_sam_device(smem if smem is not None else r.smem_opt, r.chain_opt, r.min_seed_len, r.matesw_opt, opt if opt is not None else r.sam_opt,
                                        c.idx, c.pac, pes0, id0, _seqs(r), b"", out=out)
    return types.SimpleNamespace(text=text, text_off=np.asarray(off), pes=pes, ps=c.last_pairs_sam_stats(), pt=c.last_phase2_text_stats(),
                                 mt=c.last_matesw_table_stats(), dedup=c.last_dedup_stats()[:2], chain=c.chain_stats(), driver=c.driver_stats())


def compose(c, r, id0=0, pes0=None, opt=None, smem=None, drop=False):
    """the composition the call must equal, on c: its switches set as the call runs them"""
    pkg, w, o = load_package(), pc.world(), opt if opt is not None else r.sam_opt
    level = float(o["mask_level_redun"])
    c.set_params(r.params), c.set_regs_dedup(True, level), c.set_regs_drop_exact(drop), c.set_pestat_collect(pes0 is None, o if pes0 is None else None)
    regs1 = c.seed_chain_regs_batch(smem if smem is not None else r.smem_opt, r.chain_opt, w.l_pac, r.reads, r.min_seed_len)
    dedup, chain = c.last_dedup_stats()[:2], c.chain_stats()
    dropped = c.last_drop_exact_stats() if drop else None
    pes = pkg.pestat_from_candidates(o, c.last_pestat_candidates(len(r.reads) // 2)[0]) if pes0 is None else pes0
    regs2, n_sw = c.matesw_device(w.l_pac, r.reads, regs1, pes, r.matesw_opt, level)
    c.set_region_long(True)
    text, off = c.phase2_text_device(o, c.idx, c.pac, pes, id0, _seqs(r), regs2, b"")
    return types.SimpleNamespace(text=text, text_off=np.asarray(off), pes=pes, regs1=regs1, regs2=regs2, n_sw=n_sw, pt=c.last_phase2_text_stats(), dedup=dedup,
                                 chain=chain, dropped=dropped)


def fresh(pkg, fn, *a, **kw):
    c = pc.new_context(pkg)
    try:
        return fn(c, *a, **kw)
    finally:
        c.close()


def both(pkg, r, **kw):
    """the call, then the composition, on one fresh context"""
    c = pc.new_context(pkg)
    try:
        return call(c, r, **kw), compose(c, r, **kw)
    finally:
        c.close()


def walk(o, regs2):
    """decide_table_sizes' rule over the vectors after rescue: (kmax of the regions, pair_kmax, opool_cap, total)"""
    kmax, cap, total, refused = hr.plan(o, regs2)
    assert not refused
    return kmax, pair_kmax([len(a) for a in regs2]), cap, total


def mid_bytes(ps, mt):
    """what the header says comes down between the phases: phase 1's status words and total, rescue's plan, 16 bytes a round, rescue's total
    with the plan record behind it; 4 bytes a pair where the call makes the table"""
    rounds = mt["waits"] - 2
    return 72 + 64 + 16 * rounds + 80 + (0 if ps["pes_given"] else 4 * ps["pairs"])


def assert_same_route(got, want, what, o):
    assert got.text == want.text and np.array_equal(got.text_off, want.text_off), (what, got.text[:300], want.text[:300])
    assert bits(got.pes) == bits(np.asarray(want.pes)), (what, got.pes, want.pes)
    ps = got.ps
    n = len(want.regs1)
    assert (ps["reads"], ps["pairs"]) == (n, n // 2) and ps["neg_index"] == 0 and ps["plan_ms"] == -1 and ps["mid_h2d_bytes"] == 0, (what, ps)
    assert (ps["regions_in"], ps["regions"]) == (want.dedup[0], sum(map(len, want.regs1))) and got.dedup == want.dedup, (what, ps, want.dedup)
    assert (ps["regions_out"], ps["n_sw"]) == (sum(map(len, want.regs2)), sum(want.n_sw)), (what, ps, sum(want.n_sw))
    assert (ps["kmax"], ps["pair_kmax"], ps["opool_cap"], ps["regions_out"]) == walk(o, want.regs2), (what, ps, walk(o, want.regs2))
    assert got.chain == want.chain, (what, got.chain, want.chain)
    assert ps["waits_mid"] == 1 + got.mt["waits"] and ps["mid_d2h_bytes"] == mid_bytes(ps, got.mt), (what, ps, got.mt)
    assert (got.mt["regions_in"], got.mt["regions_out"], got.mt["pairs"]) == (ps["regions"], ps["regions_out"], ps["pairs"]), (what, got.mt, ps)
    for k in P2_KEYS:
        assert got.pt[k] == want.pt[k], (what, k, got.pt, want.pt)


@pytest.fixture(scope="module")
def routes(pkg):
    """per paired-end run, each on a fresh context and computed once: the call without a table, pipechain.device_chain, the
    composition without a table, and the call and the composition under device_chain's table handed in"""
    done = {}

    def get(name):
        if name not in done:
            r = pc.run(name)
            dev = fresh(pkg, pc.device_chain, r)
            done[name] = (fresh(pkg, call, r), dev, fresh(pkg, compose, r), fresh(pkg, call, r, pes0=dev.pes), fresh(pkg, compose, r, pes0=dev.pes))
        return done[name]
    return get


# ---------------------------------------------------------------- the reference, the route, the hand-off's numbers

@pytest.mark.parametrize("name", PE)
def test_reference_parity(routes, name):
    """the reference's own SAM body, byte for byte, and its per-read offsets, out of one call"""
    pc.assert_text(routes(name)[0], pc.run(name), name + ", bmh_pairs_sam_device")


@pytest.mark.parametrize("name", PE)
def test_route_parity_and_the_hand_offs_numbers(routes, name):
    got, dev, comp, got_t, comp_t = routes(name)
    r = pc.run(name)
    assert got.text == dev.text and np.array_equal(got.text_off, dev.text_off), name
    assert bits(got.pes) == bits(dev.pes), (got.pes, dev.pes)
    assert not all(int(f) for f in got.pes["failed"])  # a table with an open orientation: rescue was live
    ps = got.ps
    assert (ps["regions_in"], ps["regions"]) == dev.stats["dedup"], (ps, dev.stats["dedup"])
    assert (ps["regions"], ps["regions_out"], ps["n_sw"]) == (sum(map(len, dev.regs1)), sum(map(len, dev.regs2)), sum(dev.n_sw)), ps
    assert ps["regions_out"] > ps["regions"] and ps["n_sw"] > 0 and ps["pes_given"] == 0  # rescue added regions
    kmax, pk, cap, total = walk(r.sam_opt, dev.regs2)
    assert (ps["kmax"], ps["pair_kmax"], ps["opool_cap"], ps["regions_out"]) == (kmax, pk, cap, total), (ps, kmax, pk, cap, total)
    assert kmax > 50 and pk >= 5 and cap > 100 * total  # (the plan looked at the regions and at the pairs)
    sl = dev.stats["slices"][0]
    for k in ("wanted", "fixed", "redone", "lines", "text_bytes"):
        assert got.pt[k] == sl[k], (k, got.pt, sl)
    assert_same_route(got, comp, name, r.sam_opt)
    assert got_t.ps["pes_given"] == 1
    assert_same_route(got_t, comp_t, name + " with the table handed in", r.sam_opt)
    assert got_t.text == got.text


@pytest.mark.parametrize("name", PE)
def test_nothing_of_the_regions_crosses(pkg, routes, name):
    """a quiet download of the regions would grow with n; a quiet upload would show in phase 2's bytes"""
    got, dev, comp, got_t, comp_t = routes(name)
    r = pc.run(name)
    pairs = len(r.reads) // 2
    assert pairs == 200
    for g, cmp_ in ((got, comp), (got_t, comp_t)):
        regions = g.ps["regions_out"]
        assert regions > len(r.reads)
        print(name, "h2d", g.pt["h2d_bytes"], "against", cmp_.pt["h2d_bytes"], "regions", regions, "mid d2h", g.ps["mid_d2h_bytes"], "waits", g.ps["waits_mid"])
        assert g.pt["h2d_bytes"] <= cmp_.pt["h2d_bytes"] - 64 * regions, (g.pt, cmp_.pt, regions)
        assert g.pt["d2h_bytes"] == cmp_.pt["d2h_bytes"], (g.pt, cmp_.pt)
        assert g.ps["waits_mid"] == 1 + g.mt["waits"] == 3 + (g.mt["waits"] - 2), (g.ps, g.mt)  # the header: 3 and one per rescue round
        assert g.ps["mid_d2h_bytes"] == mid_bytes(g.ps, g.mt), (g.ps, g.mt)
    one = pc.sub_run(r, r.reads[:2], r.names[:2], r.quals[:2])
    # with the table given: the same number for 200 pairs as for 1.  Under a table of four failed orientations no pair is active in
    # either batch, so rescue runs as many rounds -- none -- in both; under the run's own table each side owes 16 bytes per round it ran
    failed = np.zeros(4, dtype=pkg.PESTAT)
    failed["failed"] = 1
    big_f, one_f = fresh(pkg, call, r, pes0=failed), fresh(pkg, call, one, pes0=failed)
    assert big_f.ps["mid_d2h_bytes"] == one_f.ps["mid_d2h_bytes"] == 72 + 64 + 80, (big_f.ps, one_f.ps)
    assert big_f.ps["waits_mid"] == one_f.ps["waits_mid"] == 3 and big_f.ps["regions_out"] == big_f.ps["regions"] > 200
    one_t = fresh(pkg, call, one, pes0=dev.pes)
    assert got_t.ps["mid_d2h_bytes"] - 16 * (got_t.mt["waits"] - 2) == one_t.ps["mid_d2h_bytes"] - 16 * (one_t.mt["waits"] - 2) == 72 + 64 + 80, (got_t.ps, one_t.ps)
    # without one: exactly 4 bytes per pair more, the words
    one_n = fresh(pkg, call, one)
    assert got.ps["mid_d2h_bytes"] == got_t.ps["mid_d2h_bytes"] + 4 * pairs, (got.ps, got_t.ps)
    assert one_n.ps["mid_d2h_bytes"] - 16 * (one_n.mt["waits"] - 2) == 72 + 64 + 80 + 4, (one_n.ps, one_n.mt)


# ---------------------------------------------------------------- the plan kernel's block edges

def _edge_order(routes):
    """pe0's pairs in an order that puts a pair whose rescue runs Smith-Waterman at positions 0, 62, 63, 64 and 128: the last lane of a
    63-pair batch's second wave, both sides of the 64-pair edge, and the first lane of a fifth wave"""
    n_sw = routes("pe0")[1].n_sw
    live = [p for p, k in enumerate(n_sw) if k > 0]
    rest = [p for p, k in enumerate(n_sw) if k == 0]
    assert len(live) >= 5 and len(rest) >= 124, (len(live), len(rest))
    return [live[0]] + rest[:61] + live[1:4] + rest[61:124] + [live[4]]


def _pairs(r, order):
    idx = [i for p in order for i in (2 * p, 2 * p + 1)]
    return pc.sub_run(r, [r.reads[i] for i in idx], [r.names[i] for i in idx], [r.quals[i] for i in idx])


@pytest.mark.parametrize("id0", [0, 7])
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 129])
def test_block_edges(pkg, routes, n_pairs, id0):
    r = pc.run("pe0")
    table = routes("pe0")[1].pes
    x = _pairs(r, _edge_order(routes)[:n_pairs])
    c = pc.new_context(pkg)
    try:
        want_t, got_t = compose(c, x, id0, pes0=table), call(c, x, id0, pes0=table)
        want_n, got_n = compose(c, x, id0), call(c, x, id0)
    finally:
        c.close()
    # the whole run's table: rescue is live at every size
    assert sum(want_t.n_sw) > 0 and want_t.n_sw[0] > 0 and (n_pairs < 63 or want_t.n_sw[62] > 0) and (n_pairs < 129 or want_t.n_sw[128] > 0), want_t.n_sw
    assert_same_route(got_t, want_t, (n_pairs, id0, "table"), x.sam_opt)
    assert got_t.ps["n_sw"] > 0 and got_t.mt["active"] > 0
    # the batch's own table: of one pair, four failed orientations, and the session runs through all the same
    assert_same_route(got_n, want_n, (n_pairs, id0, "own table"), x.sam_opt)
    if n_pairs == 1:
        assert all(int(f) for f in got_n.pes["failed"]) and got_n.ps["n_sw"] == 0 and got_n.mt["active"] == 0 and got_n.ps["waits_mid"] == 3
    assert got_n.text.count(b"\n") >= 2 * n_pairs


def test_kernel_timing_brackets_the_plan(pkg, routes):
    """with bmh_set_kernel_timing on, the events around the plan kernel are recorded behind mate rescue and read by this caller:
    plan_ms is a duration, and the text is the untimed call's"""
    r = pc.run("pe0")
    table = routes("pe0")[1].pes
    x = _pairs(r, _edge_order(routes)[:33])
    c = pc.new_context(pkg)
    try:
        plain = call(c, x, pes0=table)
        c.set_kernel_timing(True)
        timed = call(c, x, pes0=table)
    finally:
        c.close()
    print("plan_ms", timed.ps["plan_ms"])
    assert plain.ps["plan_ms"] == -1 and timed.ps["plan_ms"] >= 0, (plain.ps, timed.ps)
    assert timed.ps["n_sw"] == plain.ps["n_sw"] > 0  # rescue was live in front of the plan
    assert timed.text == plain.text and np.array_equal(timed.text_off, plain.text_off)


# ---------------------------------------------------------------- few or no regions, one mate unalignable

def _nowhere_pairs(n_pairs, seed):
    """pairs of random reads: 100 random bases share no 19-mer with a 48 kb genome (4^19 against 10^5 of them)"""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(2 * n_pairs)]
    return reads, [b"rnd%d" % (i // 2) for i in range(2 * n_pairs)], [None] * (2 * n_pairs)


def _a_pair_with_regions(routes):
    regs1 = routes("pe0")[1].regs1
    return next(p for p in range(len(regs1) // 2) if len(regs1[2 * p]) >= 1 and len(regs1[2 * p + 1]) >= 1 and len(regs1[2 * p]) + len(regs1[2 * p + 1]) >= 3)


def _join(r, *parts):
    return pc.sub_run(r, *[sum((list(p[k]) for p in parts), []) for k in range(3)])


def _fixture_pair(r, p):
    return r.reads[2 * p:2 * p + 2], r.names[2 * p:2 * p + 2], r.quals[2 * p:2 * p + 2]


def test_a_batch_without_a_region(pkg, routes):
    r = pc.run("pe0")
    x = pc.sub_run(r, *_nowhere_pairs(70, 1))
    for pes0 in (None, routes("pe0")[1].pes):
        got, want = both(pkg, x, pes0=pes0)
        assert_same_route(got, want, "no regions", x.sam_opt)
        ps = got.ps
        assert (ps["regions_in"], ps["regions"], ps["regions_out"], ps["n_sw"], ps["kmax"], ps["pair_kmax"], ps["opool_cap"]) == (0, 0, 0, 0, 1, 1, 0), ps
        assert ps["waits_mid"] == 3 and got.mt["active"] == 0
        lines = got.text.splitlines()
        assert len(lines) == 140 and all(int(ln.split(b"\t")[1]) & 4 for ln in lines)


def test_the_last_pair_alone_has_regions(pkg, routes):
    r, p = pc.run("pe0"), _a_pair_with_regions(routes)
    x = _join(r, _nowhere_pairs(70, 2), _fixture_pair(r, p))
    got, want = both(pkg, x, pes0=routes("pe0")[1].pes)
    assert_same_route(got, want, "the last pair", x.sam_opt)
    assert all(len(a) == 0 for a in want.regs1[:140]) and len(want.regs1[140]) + len(want.regs1[141]) >= 3
    assert got.ps["pair_kmax"] == (len(want.regs2[140]) + len(want.regs2[141])) ** 2 + 1
    assert not int(got.text.splitlines()[-1].split(b"\t")[1]) & 4


def test_pair_0_alone_has_regions(pkg, routes):
    r, p = pc.run("pe0"), _a_pair_with_regions(routes)
    x = _join(r, _fixture_pair(r, p), _nowhere_pairs(64, 3))
    got, want = both(pkg, x, pes0=routes("pe0")[1].pes)
    assert_same_route(got, want, "pair 0", x.sam_opt)
    assert all(len(a) == 0 for a in want.regs1[2:]) and len(want.regs1) == 130
    assert got.ps["pair_kmax"] == (len(want.regs2[0]) + len(want.regs2[1])) ** 2 + 1 >= 10


def test_one_mate_of_every_pair_unalignable(pkg, routes):
    """every mapped pair is a rescue candidate: the mate has no region of its own, and the table is open"""
    r = pc.run("pe0")
    rnd = _nowhere_pairs(65, 4)[0]
    reads = [rnd[i] if (i & 1) == ((i >> 1) & 1) else r.reads[i] for i in range(130)]  # the first mate of even pairs, the second of odd ones
    x = pc.sub_run(r, reads, r.names[:130], [None] * 130)
    got, want = both(pkg, x, pes0=routes("pe0")[1].pes)
    assert_same_route(got, want, "one mate unalignable", x.sam_opt)
    mapped = [p for p in range(65) if len(want.regs1[2 * p]) + len(want.regs1[2 * p + 1])]
    # (a candidate's window can be empty or uncallable, so n_sw may be 0 for one; the filter's count is what says "candidate")
    assert len(mapped) >= 50 and got.mt["active"] == len(mapped), (len(mapped), got.mt)
    assert all(want.n_sw[p] == 0 for p in range(65) if p not in mapped) and sum(want.n_sw) > 0, want.n_sw
    assert got.ps["regions_out"] == got.ps["regions"]  # (random bases align nowhere: the Smith-Watermans ran and found no mate)


# ---------------------------------------------------------------- -e

def test_no_exact(pkg, routes):
    r = pc.run("pe0")
    extra = _exact_reads()
    reads = r.reads[:128] + extra
    names = r.names[:128] + [b"exact%d" % (i // 2) for i in range(len(extra))]
    x = pc.sub_run(r, reads, names, r.quals[:128] + [None] * len(extra))
    opt, smem = x.sam_opt.copy(), x.smem_opt.copy()
    opt["flag"] = int(opt["flag"]) | pkg.MEM_F_NO_EXACT
    smem["start_width"] = 2
    table = routes("pe0")[1].pes
    c = pc.new_context(pkg)
    try:
        kept = compose(c, x, opt=opt, smem=smem, drop=False, pes0=table)
        want = compose(c, x, opt=opt, smem=smem, drop=True, pes0=table)
        lost = sum(len(b) < len(a) for a, b in zip(kept.regs1, want.regs1))
        assert lost >= 10 and want.dropped == lost, (lost, want.dropped)
        got = call(c, x, opt=opt, smem=smem, pes0=table)
        assert c.last_drop_exact_stats() == want.dropped > 0
        want_n, got_n = compose(c, x, opt=opt, smem=smem, drop=True), call(c, x, opt=opt, smem=smem)
    finally:
        c.close()
    assert got.text != kept.text
    assert_same_route(got, want, "-e with the table", opt)
    assert_same_route(got_n, want_n, "-e, its own table", opt)


# ---------------------------------------------------------------- one context in turn

def test_one_context_through_the_call_and_the_other_routes_in_turn(pkg, routes):
    """stale workspaces, hints and switches: the call, device_chain, bmh_reads_sam_device on a single-end run, the call again.  The
    call leaves the three switches as device_chain set them -- de-duplication on, drop-exact off, collect on under pe0's options --
    and the words of the last collecting call as they were"""
    pe0, pe1, se0 = pc.run("pe0"), pc.run("pe1"), pc.run("se0")
    w = pc.world()
    first = routes("pe0")[0]
    c = pc.new_context(pkg)
    try:
        got = call(c, pe0)
        pc.assert_text(got, pe0, "first")
        def differs(a, b):  # (phase 2's waits and uploaded bytes depend on what the context holds already: a moved block, the log table)
            return [(k, x[k], y[k]) for x, y, keys in ((a.ps, b.ps, a.ps), (a.mt, b.mt, a.mt), (a.pt, b.pt, P2_KEYS[:-1])) for k in keys if x[k] != y[k]]
        assert differs(got, first) == []
        dev = pc.device_chain(c, pe0)
        pc.assert_text(dev, pe0, "device_chain between")
        pc.assert_text(se_call(c, se0), se0, "bmh_reads_sam_device between")
        pc.assert_text(call(c, pe1), pe1, "the other run")
        again = call(c, pe0)
        pc.assert_text(again, pe0, "again")
        assert differs(again, first) == [] and bits(again.pes) == bits(first.pes)
        assert np.array_equal(c.last_pestat_candidates(len(pe0.reads) // 2)[0], dev.cand)  # device_chain's words, not the call's
        c.set_params(pe0.params)
        regs = c.seed_chain_regs_batch(pe0.smem_opt, pe0.chain_opt, w.l_pac, pe0.reads, pe0.min_seed_len)
        assert pc.first_region_difference(regs, dev.regs1) is None  # de-duplicated at pe0's level, nothing dropped
        assert c.last_dedup_stats()[:2] == dev.stats["dedup"]
        assert np.array_equal(c.last_pestat_candidates(len(pe0.reads) // 2)[0], dev.cand)  # collect is on, under pe0's options
    finally:
        c.close()


# ---------------------------------------------------------------- refusals

def _refused(pkg, c, r, **kw):
    n = len(r.reads)
    out = {"text": C.c_void_p(0x5a5a5a5a), "text_off": np.full(n + 1, -77, dtype=np.int64), "pes": np.full(4, 9, dtype=pkg.PESTAT)}
    with pytest.raises(pkg.BmhError) as e:
        call(c, r, out=out, **kw)
    assert out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all() and (out["pes"]["low"] == 9).all()
    return e.value.code, str(e.value)


def test_refusals(pkg, routes):
    r = pc.run("pe0")
    x = pc.sub_run(r, r.reads[:130], r.names[:130], r.quals[:130])
    table = routes("pe0")[1].pes
    c = pc.new_context(pkg)
    try:
        want = compose(c, x, pes0=table)

        def fine(what):
            got = call(c, x, pes0=table)
            assert got.text == want.text and np.array_equal(got.text_off, want.text_off), what
        fine("before")
        long_pair = pc.sub_run(r, [np.zeros(65_536, dtype=np.uint8), r.reads[1]], [b"long", b"long"], [None, None])
        assert _refused(pkg, c, long_pair, pes0=table)[0] == pkg.BMH_E_RANGE
        fine("after a read past 65535 bases")
        code, why = _refused(pkg, c, pc.sub_run(r, r.reads[:4], [b"a", b"a", b"b", b"c"], [None] * 4), pes0=table)
        assert code == pkg.BMH_E_ARG
        fine("after mates with different names")
        wide = x.sam_opt.copy()
        wide["max_ins"] = 1 << 30
        code, why = _refused(pkg, c, x, opt=wide)
        assert code == pkg.BMH_E_RANGE and "max_ins" in why, why
        fine("after max_ins = 2^30 without a table")
        got, cmp_ = call(c, x, opt=wide, pes0=table), compose(c, x, opt=wide, pes0=table)  # the same options with a table given run
        assert got.text == cmp_.text and np.array_equal(got.text_off, cmp_.text_off)
        huge = np.array(table, dtype=pkg.PESTAT).copy()
        huge["failed"] = [1, 0, 1, 1]
        huge["low"][1], huge["high"][1] = 1, (1 << 20) + 1
        code, why = _refused(pkg, c, x, pes0=huge)
        assert code == pkg.BMH_E_RANGE and "pair table" in why, why
        assert c.last_dedup_stats()[:2] == want.dedup  # phase 1 had run: the refusal came after it, from a check on the host
        fine("after a pair table past 2^20 entries")
        se = x.sam_opt.copy()
        se["flag"] = int(se["flag"]) & ~pc.MEM_F_PE
        assert _refused(pkg, c, x, opt=se, pes0=table)[0] == pkg.BMH_E_ARG
        assert _refused(pkg, c, pc.sub_run(r, r.reads[:3], r.names[:3], r.quals[:3]), pes0=table)[0] == pkg.BMH_E_ARG
        fine("after a single-end flag and an odd n")
        none = call(c, pc.sub_run(r, [], [], []))  # n == 0: an empty text, text_off[0] = 0
        assert none.text == b"" and none.text_off.tolist() == [0] and none.ps["reads"] == 0 and none.ps["waits_mid"] == 0
        assert all(int(f) for f in none.pes["failed"])
        fine("after an empty batch")
    finally:
        c.close()
