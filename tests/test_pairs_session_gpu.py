"""bmh_pairs_sam_begin / bmh_pairs_sam_finish: the paired-end session cut in two at the insert-size barrier, its region table and bases
parked in a device block between the halves.  Against the reference's SAM body for the fixture's two paired-end runs (200 pairs each,
tests/golden/pipeline_golden.npz) and against the one-call form, bmh_pairs_sam_device, under the same table.

The case the one-call form cannot pass without a table handed in: the chunk cut into batches of 1, 63, 64, 65 and the remaining 7
pairs, begun on two contexts alternately, ONE table from the concatenated words, finished in reverse order each on the other context.
Over the reference's own regions (mem_align1_core on the fixture's genome, then bmh_pestat_candidates and bmh_pestat_from_candidates on
the host) every one of those five batches has a table of its own that differs from the chunk's, under both option sets: batches 0 and 4
fail all four orientations, batches 1..3 open FR with bounds (1, 581), (1, 631), (1, 546) against the chunk's (1, 572) -- pe1: (3, 577) for
batch 1.  The test asserts that difference again from the device's words before it looks at any text.

Then what a context does between a batch's two halves, block recycling with free and trim, the edge batches of
test_pairs_sam_device_gpu.py, pass C without the bases in its per-read pool (every residue of the records' 8-byte alignment and of the
bases' offsets), and the refusals that leave the handle valid."""
import ctypes as C
import types

import numpy as np
import pytest

import pipechain as pc
from __graft_entry__ import load_package
from test_pairs_sam_device_gpu import _a_pair_with_regions, _fixture_pair, _join, _nowhere_pairs, _seqs, call, fresh
from test_pestat_cand_cpu import bits
from test_reads_sam_device_gpu import _exact_reads
from test_reads_sam_device_gpu import call as se_call

pytestmark = pytest.mark.gpu

PE = ("pe0", "pe1")
CUTS = (1, 63, 64, 65)  # pairs; the rest of the 200 is the fifth batch


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def begin(c, r, opt=None, smem=None, collect=True, seqs=None):
    c.set_params(r.params), c.set_region_long(True)
    return c.pairs_sam_begin(smem if smem is not None else r.smem_opt, r.chain_opt, r.min_seed_len, opt if opt is not None else r.sam_opt, c.idx,
                             seqs if seqs is not None else _seqs(r), collect=collect)


def finish(c, r, parked, pes, id0=0, opt=None, seqs=None):
    c.set_params(r.params), c.set_region_long(True)
    text, off = c.pairs_sam_finish(parked, r.matesw_opt, opt if opt is not None else r.sam_opt, c.idx, c.pac, pes, id0, seqs if seqs is not None else _seqs(r), b"")
    return types.SimpleNamespace(text=text, text_off=np.asarray(off), ps=c.last_pairs_sam_stats(), pt=c.last_phase2_text_stats(), mt=c.last_matesw_table_stats())


def two_calls(c, r, pes=None, id0=0, opt=None, smem=None, other=None):
    """begin on c, the table from its own words unless one is given, finish on `other` or c"""
    pkg = load_package()
    parked, cand = begin(c, r, opt=opt, smem=smem)
    info = parked.info()
    table = pes if pes is not None else pkg.pestat_from_candidates(opt if opt is not None else r.sam_opt, cand)
    got = finish(other if other is not None else c, r, parked, table, id0=id0, opt=opt)
    assert parked._h is None  # consumed
    got.cand, got.pes, got.info = cand, table, info
    return got


def sub(r, lo, hi):
    return pc.sub_run(r, r.reads[lo:hi], r.names[lo:hi], r.quals[lo:hi])


def same_text(got, want, what):
    assert got.text == want.text and np.array_equal(got.text_off, want.text_off), (what, got.text[:300], want.text[:300])


@pytest.fixture(scope="module")
def whole(pkg):
    """per paired-end run, computed once: the one-call form without a table, the composition's hand-offs, the session in two calls"""
    done = {}

    def get(name):
        if name not in done:
            r = pc.run(name)
            done[name] = (fresh(pkg, call, r), fresh(pkg, pc.device_chain, r), fresh(pkg, two_calls, r))
        return done[name]
    return get


# ---------------------------------------------------------------- the whole chunk

@pytest.mark.parametrize("name", PE)
def test_whole_chunk(whole, name):
    one, dev, got = whole(name)
    r = pc.run(name)
    pc.assert_text(got, r, name + ", begin + finish")
    same_text(got, one, name)
    assert np.array_equal(got.cand, dev.cand)  # the composition's bmh_last_pestat_candidates
    assert bits(got.pes) == bits(one.pes)
    n = len(r.reads)
    assert got.info == {"device": 0, "reads": n, "regions": one.ps["regions"], "bytes": got.info["bytes"]}
    # the block: two offset arrays, the regions and the bases in 256-byte sections, 16 zero bytes behind the bases
    a = lambda x: (x + 255) & ~255  # noqa: E731
    assert got.info["bytes"] == 2 * a(8 * (n + 1)) + a(one.ps["regions"] * pc.ALNREG.itemsize) + sum(map(len, r.reads)) + 16
    ps = got.ps
    for k in ("reads", "pairs", "regions_in", "regions", "regions_out", "n_sw", "kmax", "pair_kmax", "opool_cap", "mid_d2h_bytes", "mid_h2d_bytes", "neg_index"):
        assert ps[k] == one.ps[k], (k, ps, one.ps)
    # one wait more than the one-call form's: the copy into the block behind the wait that brought the table's total
    assert ps["pes_given"] == 1 and ps["waits_mid"] == 2 + got.mt["waits"] == one.ps["waits_mid"] + 1, (ps, got.mt, one.ps)
    for k in ("units", "wanted", "fixed", "redone", "reads", "lines", "text_bytes", "d2h_bytes", "fallbacks", "sessions"):
        assert got.pt[k] == one.pt[k], (k, got.pt, one.pt)
    assert got.pt["h2d_bytes"] < one.pt["h2d_bytes"]  # (the exact difference: test_resident_bases)


# ---------------------------------------------------------------- many batches, one table, two contexts

def _batches(n_pairs):
    lo, out = 0, []
    for c in CUTS + (n_pairs - sum(CUTS),):
        out.append((2 * lo, 2 * (lo + c)))
        lo += c
    return out


@pytest.mark.parametrize("name", PE)
def test_batches_under_the_chunks_table(pkg, whole, name):
    r = pc.run(name)
    cuts = _batches(len(r.reads) // 2)
    assert cuts[-1] == (386, 400)
    ctx = [pc.new_context(pkg), pc.new_context(pkg)]
    try:
        parked, words = [], []
        for k, (lo, hi) in enumerate(cuts):
            h, cand = begin(ctx[k & 1], sub(r, lo, hi))
            parked.append(h), words.append(cand)
        cand = np.concatenate(words)
        assert np.array_equal(cand, whole(name)[1].cand)
        table = pkg.pestat_from_candidates(r.sam_opt, cand)
        assert bits(table) == bits(whole(name)[0].pes)
        for w in words:  # the case proves something: no batch's own table is the chunk's
            assert bits(pkg.pestat_from_candidates(r.sam_opt, w)) != bits(table), len(w)
        texts, offs = [None] * len(cuts), [None] * len(cuts)
        for k in reversed(range(len(cuts))):
            lo, hi = cuts[k]
            got = finish(ctx[(k + 1) & 1], sub(r, lo, hi), parked[k], table, id0=lo)
            texts[k], offs[k] = got.text, got.text_off
            assert got.ps["reads"] == hi - lo and got.ps["pes_given"] == 1
    finally:
        for c in ctx:
            c.close()
    text, at, off = b"".join(texts), 0, [np.zeros(1, dtype=np.int64)]
    for t, o in zip(texts, offs):
        off.append(o[1:] + at)
        at += len(t)
    pc.assert_text(types.SimpleNamespace(text=text, text_off=np.concatenate(off)), r, name + ", five batches under one table")


# ---------------------------------------------------------------- what the context does between the halves

def test_other_sessions_between_begin_and_finish(pkg, whole):
    """the same context runs a paired-end and a single-end one-call session on other reads between a batch's begin and finish: they
    overwrite d_c2r, d_pbase, d_msw and every block of phase 2, and the parked batch finishes with the right text"""
    pe0, pe1, se0 = pc.run("pe0"), pc.run("pe1"), pc.run("se0")
    table = whole("pe0")[0].pes
    x, y = sub(pe0, 0, 130), sub(pe1, 130, 400)
    c = pc.new_context(pkg)
    try:
        want = call(c, x, id0=0, pes0=table)
        parked, cand = begin(c, x)
        between = call(c, y)  # more reads and more regions than the parked batch
        pc.assert_text(se_call(c, se0), se0, "bmh_reads_sam_device between")
        got = finish(c, x, parked, table)
        same_text(got, want, "after other sessions")
        same_text(call(c, y), between, "the one-call form afterwards")
    finally:
        c.close()
    assert np.array_equal(cand, whole("pe0")[1].cand[:65])


# ---------------------------------------------------------------- recycling

def test_blocks_are_recycled(pkg, whole):
    """two rounds with different tables on the same contexts, a larger batch after a smaller one and back; an unfinished handle
    freed, the idle blocks trimmed, and a further round"""
    r = pc.run("pe0")
    table = whole("pe0")[0].pes
    failed = np.zeros(4, dtype=pkg.PESTAT)
    failed["failed"] = 1
    small, big = sub(r, 0, 20), sub(r, 20, 400)
    ctx = [pc.new_context(pkg), pc.new_context(pkg)]
    try:
        want = {(k, t): call(ctx[0], x, pes0=tb) for k, x in (("small", small), ("big", big)) for t, tb in (("table", table), ("failed", failed))}
        assert want["big", "table"].text != want["big", "failed"].text

        def round_(tname, tb, order):
            for k in order:
                x = small if k == "small" else big
                parked, _ = begin(ctx[0], x)
                assert parked.info()["reads"] == len(x.reads)
                same_text(finish(ctx[1], x, parked, tb), want[k, tname], (k, tname))
        round_("table", table, ("small", "big", "small"))
        round_("failed", failed, ("big", "small", "big"))
        held, _ = begin(ctx[1], big)
        loose, _ = begin(ctx[0], small)
        loose.free()  # unfinished: its block goes back to the list
        assert loose._h is None
        pkg.pairs_parked_trim(0)  # the idle blocks go back to the runtime; the held one is untouched
        same_text(finish(ctx[0], big, held, table), want["big", "table"], "held across the trim")
        round_("table", table, ("big", "small"))
        pkg.pairs_parked_trim(0)
        pkg.pairs_parked_trim(0)  # nothing idle: nothing happens
    finally:
        for c in ctx:
            c.close()


# ---------------------------------------------------------------- edge batches

def _against_one_call(pkg, x, table, what, **kw):
    c = pc.new_context(pkg)
    try:
        want = call(c, x, pes0=table, **kw)
        got = two_calls(c, x, pes=table, **kw)
    finally:
        c.close()
    same_text(got, want, what)
    for k in ("regions_in", "regions", "regions_out", "n_sw", "kmax", "pair_kmax", "opool_cap"):
        assert got.ps[k] == want.ps[k], (what, k, got.ps, want.ps)
    return got, want


def test_a_batch_without_a_region(pkg, whole):
    r = pc.run("pe0")
    x = pc.sub_run(r, *_nowhere_pairs(70, 1))
    got, _ = _against_one_call(pkg, x, whole("pe0")[0].pes, "no regions")
    assert (got.ps["regions"], got.ps["regions_out"], got.info["regions"]) == (0, 0, 0) and got.ps["waits_mid"] == 4
    assert not got.cand.any()
    lines = got.text.splitlines()
    assert len(lines) == 140 and all(int(ln.split(b"\t")[1]) & 4 for ln in lines)


def test_the_last_pair_alone_has_regions(pkg, whole):
    r = pc.run("pe0")
    routes = lambda name: (None, whole(name)[1])  # noqa: E731  (the helper wants device_chain's regs1 at [1])
    x = _join(r, _nowhere_pairs(70, 2), _fixture_pair(r, _a_pair_with_regions(routes)))
    got, _ = _against_one_call(pkg, x, whole("pe0")[0].pes, "the last pair")
    assert got.ps["regions"] >= 3 and not int(got.text.splitlines()[-1].split(b"\t")[1]) & 4


def test_no_reads(pkg, whole):
    r = pc.run("pe0")
    x = pc.sub_run(r, [], [], [])
    c = pc.new_context(pkg)
    try:
        parked, cand = begin(c, x)
        assert len(cand) == 0 and parked.info() == {"device": 0, "reads": 0, "regions": 0, "bytes": 0}
        got = finish(c, x, parked, whole("pe0")[0].pes)
        assert parked._h is None
    finally:
        c.close()
    assert got.text == b"" and got.text_off.tolist() == [0] and got.ps["reads"] == 0 and got.ps["pes_given"] == 1


def test_a_table_of_four_failed_orientations(pkg):
    r = pc.run("pe0")
    failed = np.zeros(4, dtype=pkg.PESTAT)
    failed["failed"] = 1
    got, _ = _against_one_call(pkg, sub(r, 0, 130), failed, "four failed orientations")
    assert got.ps["n_sw"] == 0 and got.mt["active"] == 0 and got.ps["regions_out"] == got.ps["regions"] > 65 and got.ps["waits_mid"] == 4


def test_no_exact(pkg, whole):
    r = pc.run("pe0")
    extra = _exact_reads()
    x = pc.sub_run(r, r.reads[:128] + extra, r.names[:128] + [b"exact%d" % (i // 2) for i in range(len(extra))], r.quals[:128] + [None] * len(extra))
    opt, smem = x.sam_opt.copy(), x.smem_opt.copy()
    opt["flag"] = int(opt["flag"]) | pkg.MEM_F_NO_EXACT
    smem["start_width"] = 2
    table = whole("pe0")[0].pes
    got, want = _against_one_call(pkg, x, table, "-e", opt=opt, smem=smem)
    plain = fresh(pkg, call, x, pes0=table, smem=smem)
    assert got.text != plain.text and got.ps["regions"] < plain.ps["regions"]  # drop-exact ran in begin


# ---------------------------------------------------------------- pass C without the bases in its pool

LENGTHS = (1, 7, 8, 9, 63, 64, 65, 250)


def _record(l_name, l_seq, qual, l_comment, bases):
    """samtext_read_bytes (csrc/samtext.h): the 16-byte header, the name, the bases where the record holds them, the qualities, the
    comment, rounded up to 8"""
    return (16 + l_name + l_seq * ((1 if bases else 0) + (1 if qual else 0)) + max(l_comment, 0) + 7) & ~7


def _mixed_pairs():
    """64 pairs over every combination of LENGTHS for the two mates, FR from the first contig 300 bases apart (mates of up to 9 bases
    have no seed and stay unaligned), every eighth pair's second mate random bases; names of 2..9 bytes, qualities on three reads of
    four, comments of 0..6 bytes on two reads of three: the records' sizes and the bases' offsets take every residue mod 8"""
    w = pc.world()
    g = np.asarray(w.genome[w.contigs[0][0]:w.contigs[0][0] + w.contigs[0][1]], dtype=np.uint8)
    rng = np.random.default_rng(11)
    seqs, i = [], 0
    for a in LENGTHS:
        for b in LENGTHS:
            p = 500 + 97 * i
            m1 = g[p:p + a].copy()
            m2 = (3 - g[p + 300:p + 300 + b][::-1]).astype(np.uint8) if i % 8 != 5 else rng.integers(0, 4, b).astype(np.uint8)
            name = b"q%d" % i + b"x" * (i % 7)
            for j, m in enumerate((m1, m2)):
                k = 2 * i + j
                qual = bytes(33 + (k + t) % 40 for t in range(len(m))) if k % 4 != 3 else None
                comment = b"c" * (k % 7) if k % 3 != 2 else None
                seqs.append((name, comment, m, qual))
            i += 1
    return seqs


def test_resident_bases(pkg, whole):
    r = pc.run("pe0")
    seqs = _mixed_pairs()
    assert {len(s[2]) for s in seqs} == set(LENGTHS)
    sizes = [[_record(len(nm), len(m), q is not None, len(cm) if cm is not None else -1, bases) for nm, cm, m, q in seqs] for bases in (True, False)]
    raw = [16 + len(nm) + len(m) * (q is not None) + (len(cm) if cm is not None else 0) for nm, cm, m, q in seqs]  # before the rounding
    assert {v % 8 for v in raw} == set(range(8)) and {int(v) % 8 for v in np.cumsum([len(s[2]) for s in seqs])} == set(range(8))
    x = pc.sub_run(r, [s[2] for s in seqs], [s[0] for s in seqs], [s[3] for s in seqs])
    table = whole("pe0")[0].pes
    c1, c2 = pc.new_context(pkg), pc.new_context(pkg)
    try:
        c1.set_params(x.params), c1.set_region_long(True)
        text, off, _ = c1.pairs_sam_device(x.smem_opt, x.chain_opt, x.min_seed_len, x.matesw_opt, x.sam_opt, c1.idx, c1.pac, table, 0, seqs, b"")
        want_pt, want_ps = c1.last_phase2_text_stats(), c1.last_pairs_sam_stats()
        parked, _ = begin(c2, x, seqs=seqs)
        got = finish(c2, x, parked, table, seqs=seqs)
    finally:
        c1.close(), c2.close()
    assert got.text == text and np.array_equal(got.text_off, np.asarray(off))
    lines = got.text.splitlines()
    assert len(lines) >= len(seqs) and sum(not int(ln.split(b"\t")[1]) & 4 for ln in lines) >= 40  # the long mates aligned
    assert got.ps["n_sw"] == want_ps["n_sw"] > 0 and got.ps["mid_h2d_bytes"] == 0
    # the upload is smaller by exactly the two pools' difference; a pool lies in its block in 64-byte steps, as every section does
    a64 = lambda v: (v + 63) & ~63  # noqa: E731
    saved = a64(sum(sizes[0])) - a64(sum(sizes[1]))
    print("per-read pool", sum(sizes[0]), "->", sum(sizes[1]), "bytes; h2d", want_pt["h2d_bytes"], "->", got.pt["h2d_bytes"])
    assert saved >= sum(len(s[2]) for s in seqs) - 8 * len(seqs) - 64
    assert got.pt["h2d_bytes"] == want_pt["h2d_bytes"] - saved, (got.pt, want_pt, saved)
    for k in ("wanted", "fixed", "redone", "lines", "text_bytes", "d2h_bytes", "waits"):
        assert got.pt[k] == want_pt[k], (k, got.pt, want_pt)


# ---------------------------------------------------------------- refusals that leave the handle valid

def _refused(c, x, parked, table, **kw):
    with pytest.raises(load_package().BmhError) as e:
        finish(c, x, parked, table, **kw)
    assert parked._h is not None and parked.info()["reads"] > 0  # still valid
    return e.value.code, str(e.value)


def test_refusals_leave_the_handle_valid(pkg, whole):
    r = pc.run("pe0")
    table = whole("pe0")[0].pes
    x = sub(r, 0, 130)
    c = pc.new_context(pkg)
    try:
        want = call(c, x, pes0=table)
        parked, _ = begin(c, x)
        code, why = _refused(c, sub(r, 0, 128), parked, table)  # another n
        assert code == pkg.BMH_E_ARG and "130" in why, why
        shorter = pc.sub_run(r, r.reads[:129] + [r.reads[129][:-1]], r.names[:130], r.quals[:129] + [r.quals[129][:-1]])
        code, why = _refused(c, shorter, parked, table)  # the same n, a read one base shorter
        assert code == pkg.BMH_E_ARG and "read 129" in why, why
        renamed = pc.sub_run(r, r.reads[:130], r.names[:128] + [b"a", b"b"], r.quals[:130])
        assert _refused(c, renamed, parked, table)[0] == pkg.BMH_E_ARG  # what phase 2 refuses of its arguments: mates named differently
        huge = np.array(table, dtype=pkg.PESTAT).copy()
        huge["failed"] = [1, 0, 1, 1]
        huge["low"][1], huge["high"][1] = 1, (1 << 20) + 1
        code, why = _refused(c, x, parked, huge)  # the pair table's refusal, before rescue
        assert code == pkg.BMH_E_RANGE and "pair table" in why, why
        same_text(finish(c, x, parked, table), want, "after four refusals")
        assert parked._h is None
    finally:
        c.close()


def test_a_context_of_another_device_is_refused(pkg, whole):
    ndev = C.c_int(0)
    assert pkg.lib().bmh_device_count(C.byref(ndev)) == 0
    if ndev.value < 2:
        pytest.skip("one visible device: a parked block has no other device to be refused on")
    r = pc.run("pe0")
    table = whole("pe0")[0].pes
    x = sub(r, 0, 20)
    w = pc.world()
    c, far = pc.new_context(pkg), pkg.Context(1)
    try:
        far.pac = far.set_pac(w.pac, w.l_pac)
        far.idx = pkg.make_refidx(w.contigs, w.l_pac, w.names)
        far.set_refidx(far.idx), far.set_refnames(far.idx)
        want = call(c, x, pes0=table)
        parked, _ = begin(c, x)
        code, why = _refused(far, x, parked, table)
        assert code == pkg.BMH_E_ARG and "device" in why, why
        same_text(finish(c, x, parked, table), want, "after the other device's refusal")
    finally:
        c.close(), far.close()
