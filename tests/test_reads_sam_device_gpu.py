"""bmh_reads_sam_device: single-end reads to SAM text with the region vectors on the device from the kernel that makes them to the
kernel that sorts them.  Against the compiled reference's SAM body for the fixture's two single-end runs (tests/pipechain.py over
tests/golden/pipeline_golden.npz), against the two-call composition it replaces (bmh_seed_chain_regs_batch, then
bmh_phase2_text_device) text for text and number for number, and against the conditions a quiet download or upload of the regions
would break: the hand-off's bytes do not depend on n, phase 2 uploads at least 64 bytes per region less than the composition and
downloads as much.  Then the block edges of table_plan_kernel, its events in timing mode, batches with few or no regions, -e, one context through the call and
the other route in turn, and the refusals."""
import ctypes as C
import types

import numpy as np
import pytest

import handoff_ref as hr
import pipechain as pc
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

SE = ("se0", "se1")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def _seqs(r):
    return [(r.names[i], None, r.reads[i], r.quals[i]) for i in range(len(r.reads))]


def call(c, r, id0=0, opt=None, smem=None, out=None):
    """the call on c, and what its statistics and the other calls' say afterwards"""
    c.set_params(r.params), c.set_region_long(True)
    text, off = c.reads_sam_device(smem if smem is not None else r.smem_opt, r.chain_opt, r.min_seed_len, opt if opt is not None else r.sam_opt, c.idx, c.pac,
                                   id0, _seqs(r), b"", out=out)
    return types.SimpleNamespace(text=text, text_off=np.asarray(off), rs=c.last_reads_sam_stats(), pt=c.last_phase2_text_stats(), dedup=c.last_dedup_stats()[:2],
                                 driver=c.driver_stats(), chain=c.chain_stats())


def compose(c, r, id0=0, opt=None, smem=None, drop=False):
    """the composition the call must equal, on c: its switches set as the call runs them"""
    w, o = pc.world(), opt if opt is not None else r.sam_opt
    c.set_params(r.params), c.set_regs_dedup(True, float(o["mask_level_redun"])), c.set_regs_drop_exact(drop), c.set_pestat_collect(False)
    regs1 = c.seed_chain_regs_batch(smem if smem is not None else r.smem_opt, r.chain_opt, w.l_pac, r.reads, r.min_seed_len)
    dedup, driver, chain = c.last_dedup_stats()[:2], c.driver_stats(), c.chain_stats()
    dropped = c.last_drop_exact_stats() if drop else None
    c.set_region_long(True)
    text, off = c.phase2_text_device(o, c.idx, c.pac, None, id0, _seqs(r), regs1, b"")
    return types.SimpleNamespace(text=text, text_off=np.asarray(off), regs1=regs1, pt=c.last_phase2_text_stats(), dedup=dedup, driver=driver, chain=chain,
                                 dropped=dropped)


def fresh(pkg, fn, *a, **kw):
    c = pc.new_context(pkg)
    try:
        return fn(c, *a, **kw)
    finally:
        c.close()


def assert_same_route(got, want, what, n_regs=None):
    assert got.text == want.text and np.array_equal(got.text_off, want.text_off), (what, got.text[:300], want.text[:300])
    total = sum(map(len, want.regs1))
    assert (got.rs["regions_in"], got.rs["regions"]) == (want.dedup[0], total) and got.dedup == want.dedup, (what, got.rs, want.dedup, total)
    assert got.rs["waits_tail"] == 1 + want.pt["waits"] and got.pt["waits"] == want.pt["waits"], (what, got.rs, want.pt)
    assert got.driver == want.driver and got.chain == want.chain, (what, got.driver, want.driver, got.chain, want.chain)
    for k in ("units", "wanted", "fixed", "redone", "reads", "lines", "text_bytes", "d2h_bytes", "fallbacks", "sessions"):
        assert got.pt[k] == want.pt[k], (what, k, got.pt, want.pt)
    assert got.rs["neg_index"] == 0 and got.rs["reads"] == len(want.regs1) and got.rs["plan_ms"] == -1


@pytest.fixture(scope="module")
def routes(pkg):
    """per single-end run, each on a fresh context and computed once: the call, pipechain.device_chain, and the composition"""
    done = {}

    def get(name):
        if name not in done:
            r = pc.run(name)
            done[name] = (fresh(pkg, call, r), fresh(pkg, pc.device_chain, r), fresh(pkg, compose, r))
        return done[name]
    return get


# ---------------------------------------------------------------- the reference, the route, the hand-off's numbers

@pytest.mark.parametrize("name", SE)
def test_reference_parity(routes, name):
    """the reference's own SAM body, byte for byte, and its per-read offsets"""
    pc.assert_text(routes(name)[0], pc.run(name), name + ", bmh_reads_sam_device")


@pytest.mark.parametrize("name", SE)
def test_route_parity_and_the_hand_offs_numbers(routes, name):
    got, dev, comp = routes(name)
    r = pc.run(name)
    assert got.text == dev.text and np.array_equal(got.text_off, dev.text_off), name
    assert (got.rs["regions_in"], got.rs["regions"]) == dev.stats["dedup"], (got.rs, dev.stats["dedup"])
    kmax, cap, total, refused = hr.plan(r.sam_opt, dev.regs1)
    assert not refused and got.rs["neg_index"] == 0
    assert (got.rs["kmax"], got.rs["opool_cap"], got.rs["regions"]) == (kmax, cap, total), (got.rs, kmax, cap, total)
    assert kmax > 50 and cap > 100 * total  # (a length past mapQ_coef_len decides kmax: the plan looked at the regions)
    assert got.rs["waits_tail"] == 1 + dev.stats["slices"][0]["waits"], (got.rs, dev.stats["slices"][0])
    assert dev.stats["slices"][0]["redone"] >= 1  # the redo ran, from the list's own records
    assert_same_route(got, comp, name)


@pytest.mark.parametrize("name", SE)
def test_nothing_of_the_regions_crosses(pkg, routes, name):
    """a quiet download of the regions would grow with n; a quiet upload would show in phase 2's bytes"""
    got, dev, comp = routes(name)
    r = pc.run(name)
    one = fresh(pkg, call, pc.sub_run(r, r.reads[:1], r.names[:1], r.quals[:1]))
    assert one.rs["handoff_d2h_bytes"] == got.rs["handoff_d2h_bytes"] <= 256, (one.rs, got.rs)
    regions = got.rs["regions"]
    assert regions > len(r.reads) == 190
    assert got.pt["d2h_bytes"] == comp.pt["d2h_bytes"], (got.pt, comp.pt)
    print(name, "h2d", got.pt["h2d_bytes"], "against", comp.pt["h2d_bytes"], "regions", regions)
    assert got.pt["h2d_bytes"] <= comp.pt["h2d_bytes"] - 64 * regions, (got.pt, comp.pt, regions)


# ---------------------------------------------------------------- the plan kernel's block edges

@pytest.mark.parametrize("id0", [0, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_block_edges(pkg, n, id0):
    r = pc.run("se0")
    x = pc.sub_run(r, r.reads[:n], r.names[:n], r.quals[:n])
    c = pc.new_context(pkg)
    try:
        want, got = compose(c, x, id0), call(c, x, id0)
    finally:
        c.close()
    assert_same_route(got, want, (n, id0))
    kmax, cap, total, _ = hr.plan(x.sam_opt, want.regs1)
    assert (got.rs["kmax"], got.rs["opool_cap"], got.rs["regions"]) == (kmax, cap, total)
    assert got.text.count(b"\n") >= n


def test_kernel_timing_brackets_the_plan(pkg):
    """with bmh_set_kernel_timing on, the events around the plan kernel are recorded and read from this caller: plan_ms is a duration,
    and the text is the untimed call's"""
    r = pc.run("se0")
    x = pc.sub_run(r, r.reads[:65], r.names[:65], r.quals[:65])
    c = pc.new_context(pkg)
    try:
        plain = call(c, x)
        c.set_kernel_timing(True)
        timed = call(c, x)
    finally:
        c.close()
    print("plan_ms", timed.rs["plan_ms"])
    assert plain.rs["plan_ms"] == -1 and timed.rs["plan_ms"] >= 0, (plain.rs, timed.rs)
    assert timed.text == plain.text and np.array_equal(timed.text_off, plain.text_off)


# ---------------------------------------------------------------- few or no regions

def _nowhere(n, seed):
    """n random reads: 100 random bases share no 19-mer with a 48 kb genome (4^19 against 10^5 of them)"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, 100).astype(np.uint8) for _ in range(n)], [b"rnd%d" % i for i in range(n)], [None] * n


def _a_read_with_regions(routes):
    regs1 = routes("se0")[1].regs1
    return next(i for i, a in enumerate(regs1) if len(a) >= 2)


def test_a_batch_without_a_region(pkg):
    r = pc.run("se0")
    x = pc.sub_run(r, *_nowhere(70, 1))
    c = pc.new_context(pkg)
    try:
        want, got = compose(c, x), call(c, x)
    finally:
        c.close()
    assert_same_route(got, want, "no regions")
    assert got.rs["regions"] == 0 and got.rs["regions_in"] == 0 and got.rs["kmax"] == 1 and got.rs["opool_cap"] == 0
    assert got.rs["waits_tail"] == 3, got.rs
    lines = got.text.splitlines()
    assert len(lines) == 70 and all(int(ln.split(b"\t")[1]) & 4 for ln in lines)


def test_the_last_read_alone_has_regions(pkg, routes):
    r, i = pc.run("se0"), _a_read_with_regions(routes)
    reads, names, quals = _nowhere(70, 2)
    x = pc.sub_run(r, reads + [r.reads[i]], names + [r.names[i]], quals + [r.quals[i]])
    c = pc.new_context(pkg)
    try:
        want, got = compose(c, x), call(c, x)
    finally:
        c.close()
    assert_same_route(got, want, "the last read")
    assert got.rs["regions"] == len(want.regs1[70]) >= 2 and all(len(a) == 0 for a in want.regs1[:70])
    assert not int(got.text.splitlines()[-1].split(b"\t")[1]) & 4


def test_read_0_alone_has_regions(pkg, routes):
    r, i = pc.run("se0"), _a_read_with_regions(routes)
    reads, names, quals = _nowhere(64, 3)
    x = pc.sub_run(r, [r.reads[i]] + reads, [r.names[i]] + names, [r.quals[i]] + quals)
    c = pc.new_context(pkg)
    try:
        want, got = compose(c, x), call(c, x)
    finally:
        c.close()
    assert_same_route(got, want, "read 0")
    assert got.rs["regions"] == len(want.regs1[0]) >= 2 and all(len(a) == 0 for a in want.regs1[1:]) and len(want.regs1) == 65
    kmax, cap, _, _ = hr.plan(x.sam_opt, want.regs1)
    assert (got.rs["kmax"], got.rs["opool_cap"]) == (kmax, cap)


# ---------------------------------------------------------------- -e

def _exact_reads(n=20, length=100, k=32):
    """n error-free reads cut from the genome, each holding at least k bases that occur a second time in it (either strand): with
    MEM_F_NO_EXACT seeding starts at two occurrences, so a read of unique sequence has no seed at all, and these have one; their own
    locus gives the full-length exact match that -e discards."""
    w = pc.world()
    g = np.ascontiguousarray(w.genome, dtype=np.uint8)
    mers = lambda a: [x.tobytes() for x in np.lib.stride_tricks.sliding_window_view(a, k)]  # noqa: E731
    seen = {}
    for m in mers(g) + mers((3 - g[::-1]).astype(np.uint8)):
        seen[m] = seen.get(m, 0) + 1
    cs = np.concatenate([[0], np.cumsum([seen[m] >= 2 for m in mers(g)])])
    ok = [s for off, ln in w.contigs for s in range(off, off + ln - length + 1) if cs[s + length - k + 1] - cs[s] > 0]
    assert len(ok) > 1000
    return [g[s:s + length].copy() for s in ok[::len(ok) // n][:n]]


def test_no_exact(pkg):
    r = pc.run("se0")
    extra = _exact_reads()
    reads, names, quals = r.reads + extra, r.names + [b"exact%d" % i for i in range(len(extra))], r.quals + [None] * len(extra)
    x = pc.sub_run(r, reads, names, quals)
    opt, smem = x.sam_opt.copy(), x.smem_opt.copy()
    opt["flag"] = int(opt["flag"]) | pkg.MEM_F_NO_EXACT
    smem["start_width"] = 2
    c = pc.new_context(pkg)
    try:
        kept = compose(c, x, opt=opt, smem=smem, drop=False)
        want = compose(c, x, opt=opt, smem=smem, drop=True)
        lost = sum(len(b) < len(a) for a, b in zip(kept.regs1, want.regs1))
        assert lost >= 10 and want.dropped == lost, (lost, want.dropped)
        got = call(c, x, opt=opt, smem=smem)
        assert c.last_drop_exact_stats() == want.dropped > 0
    finally:
        c.close()
    assert got.text != kept.text
    assert got.text == want.text and np.array_equal(got.text_off, want.text_off)
    assert (got.rs["regions_in"], got.rs["regions"]) == (want.dedup[0], sum(map(len, want.regs1))), (got.rs, want.dedup)
    assert got.rs["waits_tail"] == 1 + want.pt["waits"] and got.driver == want.driver and got.chain == want.chain


# ---------------------------------------------------------------- one context in turn

def test_one_context_through_the_call_and_the_other_route_in_turn(pkg, routes):
    """stale workspaces, hints and switches: each text must be the reference's, and the call leaves the three switches as
    device_chain set them for the paired-end run -- de-duplication on, drop-exact off, collect on"""
    se0, pe0, se1 = pc.run("se0"), pc.run("pe0"), pc.run("se1")
    w = pc.world()
    c = pc.new_context(pkg)
    try:
        pc.assert_text(call(c, se0), se0, "first")
        dev = pc.device_chain(c, pe0)
        pc.assert_text(dev, pe0, "device_chain between")
        got = call(c, se1)
        pc.assert_text(got, se1, "after it")
        assert got.rs == routes("se1")[0].rs
        c.set_params(pe0.params)  # (the scoring is not among the switches: se1's is in place)
        regs = c.seed_chain_regs_batch(pe0.smem_opt, pe0.chain_opt, w.l_pac, pe0.reads, pe0.min_seed_len)
        assert pc.first_region_difference(regs, dev.regs1) is None  # de-duplicated at pe0's level, nothing dropped
        assert c.last_dedup_stats()[:2] == dev.stats["dedup"]
        assert np.array_equal(c.last_pestat_candidates(len(pe0.reads) // 2)[0], dev.cand)  # collect is on, under pe0's options
        pc.assert_text(call(c, se0), se0, "again")
    finally:
        c.close()


# ---------------------------------------------------------------- refusals

def _refused(pkg, c, r, n_out, **kw):
    out = {"text": C.c_void_p(0x5a5a5a5a), "text_off": np.full(n_out + 1, -77, dtype=np.int64)}
    with pytest.raises(pkg.BmhError) as e:
        call(c, r, out=out, **kw)
    assert out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all()
    return e.value.code


def test_refusals(pkg, routes):
    r = pc.run("se0")
    x = pc.sub_run(r, r.reads[:65], r.names[:65], r.quals[:65])
    want = routes("se0")[0]
    end = int(want.text_off[65])
    c = pc.new_context(pkg)
    try:
        def fine(what):
            got = call(c, x)
            assert got.text == want.text[:end] and np.array_equal(got.text_off, want.text_off[:66]), what
        fine("before")
        pe = x.sam_opt.copy()
        pe["flag"] = int(pe["flag"]) | pc.MEM_F_PE
        assert _refused(pkg, c, pc.sub_run(r, r.reads[:64], r.names[:64], r.quals[:64]), 64, opt=pe) == pkg.BMH_E_ARG
        fine("after a paired-end flag")
        assert _refused(pkg, c, pc.sub_run(r, r.reads[:65], r.names[:40] + [None] + r.names[41:65], r.quals[:65]), 65) == pkg.BMH_E_ARG
        fine("after a read without a name")
        c.set_refnames(None)
        assert _refused(pkg, c, x, 65) == pkg.BMH_E_ARG
        c.set_refnames(c.idx)
        fine("after a context without names")
        long_read = pc.sub_run(r, [np.zeros(65_536, dtype=np.uint8)], [b"long"], [None])
        assert _refused(pkg, c, long_read, 1) == pkg.BMH_E_RANGE
        fine("after a read past 65535 bases")
        # n == 0: an empty text, text_off[0] = 0
        none = call(c, pc.sub_run(r, [], [], []))
        assert none.text == b"" and none.text_off.tolist() == [0] and none.rs["reads"] == 0 and none.rs["waits_tail"] == 0
        fine("after an empty batch")
    finally:
        c.close()
