"""bmh_phase2_text_device -- passes A, B and C of phase 2 as one device session: the regions and reads up once, only SAM text down --
against the host composition bmh_decide_batch, then bmh_wanted_cigar_batch, then bmh_sam_text_batch on copies of the vectors: the text
and text_off byte for byte.  Slices of tests/phase2gen.py at the kernels' block sizes, dressed with names, comments and qualities;
reads of unequal length next to each other (reads_gather_kernel's tails); regions bwa_fix_xref2 moves; alignments that outgrow their
slots and are redone on the host without sending the slice there -- also where their overflow area outgrows the block and the live
session moves it, around the 256-lane blocks of the bind and patch kernels, in pairs, and through the switch (tests/redogen.py);
every refusal with the outputs untouched; the session's transfers and waits in numbers; and the switch behind bmh_sam_batch."""
import ctypes as C

import numpy as np
import pytest

import decidegen as dg
import kswgen
import kswlib
import phase2gen as pg
import redogen
import samtextgen as sg
import wantgen as wg
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -3, -4
RG = b"rg7"


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ref():
    return wg.reference()


def _context(pkg, contigs, pac, l_pac, tables=("set_refidx", "set_refnames"), params=True):
    c = pkg.Context(0, kswlib.make_params()) if params else pkg.Context(0)
    c.idx = pkg.make_refidx(contigs)
    c.pac = c.set_pac(pac, l_pac) if pac is not None else None
    for f in tables:
        getattr(c, f)(c.idx)
    return c


@pytest.fixture(scope="module")
def ctx(pkg, ref):
    c = _context(pkg, wg.CONTIGS, ref[1], wg.L_PAC)
    yield c
    c.close()


def _dress(reads, pe):
    """names, comments and qualities as test_samtext_device_gpu.py::_phase2_slice gives them"""
    return [(b"q%d" % (i // 2 if pe else i), b"c" if i % 2 else None, np.asarray(r, dtype=np.uint8), bytes([40 + i % 30]) * len(r) if i % 5 else None)
            for i, r in enumerate(reads)]


def _is_pe(o):
    return bool(int(o["flag"]) & pg.PE)


def _host(pkg, c, o, pes, id0, seqs, vectors, rg=RG):
    """the yardstick: bmh_decide_batch, bmh_wanted_cigar_batch and bmh_sam_text_batch, on copies of the vectors"""
    a = pkg.decide_batch(o, c.idx.l_pac, pes, id0, vectors)
    res, cig, md = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), [s[2] for s in seqs], a["regs"], [list(k) for k in a["want"]], device=False)
    text, off = pkg.sam_text_batch(o, c.idx, pes, seqs, a["regs"], a, res, cig, md, rg)
    return text, off, a, res


def _same_text(dt, doff, ht, hoff, what):
    assert np.array_equal(hoff, doff), (what, np.flatnonzero(hoff != doff)[:5])
    if dt != ht:
        i = next(i for i in range(len(hoff) - 1) if dt[int(hoff[i]):int(hoff[i + 1])] != ht[int(hoff[i]):int(hoff[i + 1])])
        raise AssertionError((what, i, dt[int(hoff[i]):int(hoff[i + 1])][:400], ht[int(hoff[i]):int(hoff[i + 1])][:400]))


def _both(pkg, c, o, pes, id0, seqs, vectors, what, rg=RG, host=None, expect_waits=None):
    vecs = [np.ascontiguousarray(v, dtype=kswlib.ALNREG).reshape(-1).copy() for v in vectors]
    before = [v.tobytes() for v in vecs]
    ht, hoff, a, res = host or _host(pkg, c, o, pes, id0, seqs, vecs, rg)
    assert [v.tobytes() for v in vecs] == before  # (the yardstick works on copies)
    dt, doff = c.phase2_text_device(o, c.idx, c.pac, pes, id0, seqs, vecs, rg)
    assert [v.tobytes() for v in vecs] == before, what  # read only: not sorted, not marked
    _same_text(dt, doff, ht, hoff, what)
    st = c.last_phase2_text_stats()
    n = len(seqs)
    got = (st["units"], st["wanted"], st["reads"], st["lines"], st["text_bytes"], st["fallbacks"], st["sessions"])
    assert got == (n // 2 if _is_pe(o) else n, len(res), n, ht.count(b"\n"), len(ht), 0, 1), (what, st)
    # (no region at all: pass B has nothing to wait for; expect_waits: 7 where the overflow area is to outgrow the block)
    assert st["waits"] == (expect_waits if expect_waits is not None else 6 if st["redone"] else 4 if any(len(v) for v in vecs) else 2), (what, st)
    return (ht, hoff, a, res), st


def _with_w(c, w):
    c.set_params(kswlib.make_params(w=w))


@pytest.mark.parametrize("w", [100, 5])
@pytest.mark.parametrize("mode", ["se", "pe"])
@pytest.mark.parametrize("units", [1, 63, 64, 65, 130])
def test_unit_counts(pkg, ctx, units, mode, w):
    """decide_kernel's 64-lane blocks and the size kernel's 256: one unit, around a block, two blocks and a little"""
    o, pes, id0, reads, vectors = pg.make(mode, units=units, w=w)
    _with_w(ctx, w)
    try:
        _both(pkg, ctx, o, pes, id0, _dress(reads, mode == "pe"), vectors, f"{units} units, {mode}, w={w}")
    finally:
        _with_w(ctx, 100)


@pytest.mark.parametrize("w", [100, 5])
@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
@pytest.mark.parametrize("n_wanted", [1, 255, 256, 257, 1023, 1024, 1025, 1500])
def test_wanted_counts(pkg, ctx, n_wanted, mode, w):
    """the bind kernel's 256-lane blocks and the scans' 1024-lane tiles: one region, around a block, around a tile, two tiles"""
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=n_wanted, w=w)
    _with_w(ctx, w)
    try:
        _, st = _both(pkg, ctx, o, pes, id0, _dress(reads, mode.startswith("pe")), vectors, f"{n_wanted} wanted, {mode}, w={w}")
    finally:
        _with_w(ctx, 100)
    assert st["wanted"] == n_wanted and st["redone"] == 0 and st["waits"] == 4


@pytest.mark.parametrize("mode", ["se", "pe"])
def test_reads_of_unequal_length(pkg, ctx, ref, mode):
    """l_seq 1, 7, 8, 9, 63, 64, 65 and 250 next to each other, some without qualities or comment: the per-read tails of
    reads_gather_kernel (fewer bytes than lanes, one wave's worth and one more, four strides less a few) and the pool's 8-byte rounding.
    The longer reads carry a wanted region each, so pass B aligns what the kernel gathered."""
    whole = ref[0]
    reads, vectors = [], []
    for rep in range(3):
        for k, ln in enumerate((1, 7, 8, 9, 63, 64, 65, 250)):
            pos = 100 + 331 * rep + 40 * k
            rev = bool((k + rep) & 1)
            rd = whole[pos:pos + ln].copy()
            rb, re = wg.on_strand(pos, pos + ln, rev)
            if ln >= 63:
                a = wg.region(0, ln, rb, re, ln, 100, ln)
                a["seedcov"] = ln // 2
                vectors.append(np.array([a], dtype=kswlib.ALNREG))
            elif ln == 7:  # a region nobody wants
                a = wg.region(0, ln, rb, re, ln, 100, ln)
                vectors.append(np.array([a], dtype=kswlib.ALNREG))
            else:
                vectors.append(np.zeros(0, dtype=kswlib.ALNREG))
            reads.append(wg.revcomp(rd) if rev else rd)
    pe = mode == "pe"
    seqs = [(b"u%d" % (i // 2 if pe else i), (b"cm%d" % i) if i % 3 == 0 else None, r, bytes([36 + i % 50]) * len(r) if i % 4 != 1 else None)
            for i, r in enumerate(reads)]
    assert sorted({len(sg.pack_reads(seqs[i:i + 1])[1]) % 16 for i in range(len(seqs))}) == [0, 8]  # records end on and off a 16-byte line
    o, pes = pg.opt(100, pg.PE if pe else 0), (pg.pes_fr() if pe else None)
    _, st = _both(pkg, ctx, o, pes, 90, seqs, vectors, "unequal reads " + mode)
    assert st["wanted"] >= 6 and st["redone"] == 0


def _behind(rng, whole, rd, reg):
    """(read, vector) with the constructed region first and an ordinary region of the same read, 25 points better, second: the sort
    moves the constructed one back (tests/test_phase2_device_gpu.py)"""
    seg, rb, re, truesc, w = wg.segment(rng, whole, "exact", 70)
    n = len(rd)
    other = wg.region(n, n + len(seg), rb, re, truesc, w, int(reg["score"]) + 25)
    other["seedcov"] = 30
    reg = reg.copy()
    reg["seedcov"] = 30
    return np.concatenate([rd, seg]), np.array([reg, other], dtype=kswlib.ALNREG)


def test_fix_round_behind_the_sort(pkg, ctx, ref):
    """wantgen.overhangs' regions, each first in a vector whose other region scores higher: the sort moves them, the session fixes them"""
    whole = ref[0]
    rng = np.random.default_rng(8)
    cases = wg.overhangs(whole)
    fr, fv = pg.se_slice(rng, whole, 40)
    reads, vectors = list(fr[:20]), list(fv[:20])
    for name, rd, reg, expect in cases:
        b, v = _behind(rng, whole, rd, reg)
        reads.append(b), vectors.append(v)
    reads += fr[20:]
    vectors += fv[20:]
    _, st = _both(pkg, ctx, pg.opt(), None, 300, _dress(reads, False), vectors, "overhangs")
    n_fix = sum(c[3] != "none" for c in cases)
    assert n_fix >= 32 and st["fixed"] == n_fix and st["redone"] == 0, (n_fix, st)


def _long_reference(pkg, seed, l_pac):
    whole = kswgen.rand_seq(np.random.default_rng(seed), l_pac)
    return whole, _context(pkg, [(0, l_pac // 2), (l_pac // 2, l_pac - l_pac // 2)], wg.pack(whole), l_pac)


def _outgrowing(whole, rng, l_pac=20000):
    """the slice of test_alignments_that_outgrow_the_slots_are_redone_from_the_sorted_block (tests/test_phase2_device_gpu.py): 24 reads, of
    which four have an MD past the 128 bytes of its slot and four a CIGAR past 24 words, each of the eight the second region of its input
    vector and the first after the sort; l_pac: of the reference `whole` is (at least 18 000 bases in its first sequence)"""
    reads, vectors, special = [], [], []
    for k in range(24):
        pos = 500 + 700 * k
        if k % 6 == 2:  # long MD
            rd = whole[pos:pos + 250].copy()
            rd[::3] = (rd[::3] + 1) & 3
            tl = 250
        elif k % 6 == 4:  # long CIGAR: alternately a base deleted and a base inserted, 14 times, 30 bases apart
            parts, at = [], pos
            for j in range(14):
                parts.append(whole[at:at + 30])
                at += 30
                if j % 2:
                    parts.append(np.array([(int(whole[at]) + 2) & 3, (int(whole[at]) + 1) & 3], dtype=np.uint8))
                else:
                    at += 2
            parts.append(whole[at:at + 30])
            rd, tl = np.concatenate(parts), at + 30 - pos
        else:
            rd = kswgen.mutate(rng, whole[pos:pos + 150], sub=0.02)
            tl = 150
        rev = bool(k & 1)
        rb, re = (pos, pos + tl) if not rev else (2 * l_pac - pos - tl, 2 * l_pac - pos)
        rd = wg.revcomp(rd) if rev else rd
        reg = wg.region(0, len(rd), rb, re, len(rd) - 40, 100, len(rd) - 40)
        reg["seedcov"] = 60
        if k % 6 in (2, 4):  # behind a lower-scoring region of the same read, 120 bases from another place
            opos = 17000 + 100 * (k // 6)
            seg = whole[opos:opos + 120].copy()
            other = wg.region(0, 120, opos, opos + 120, 110, 100, 100)
            other["seedcov"] = 60
            reg["qb"], reg["qe"] = 120, 120 + len(rd)
            reads.append(np.concatenate([seg, rd])), vectors.append(np.array([other, reg], dtype=kswlib.ALNREG))
            special.append(k)
        else:
            reads.append(rd), vectors.append(np.array([reg], dtype=kswlib.ALNREG))
    return reads, vectors, special


def test_alignments_that_outgrow_the_slots_are_redone_without_sending_the_slice_to_the_host(pkg):
    whole, c = _long_reference(pkg, 60, 20000)
    try:
        reads, vectors, special = _outgrowing(whole, np.random.default_rng(61))
        (_, _, a, res), st = _both(pkg, c, pg.opt(), None, 50, _dress(reads, False), vectors, "long MD and CIGAR")
        assert len(special) == 8 and (st["redone"], st["waits"], st["fallbacks"], st["wanted"], st["fixed"]) == (8, 6, 0, 32, 0), st
        assert int((res["md_len"] > 128).sum()) == 4 and int((res["n_cigar"] > 24).sum()) == 4
        # the list, 112 bytes per region, and one more status: nothing else of passes A and B came down
        assert st["d2h_bytes"] <= st["text_bytes"] + 8 * (len(reads) + 1) + 256 + 8 * 112 + 32, st
        # the next slice on the same context is an ordinary one again
        o, pes, id0, r2, v2 = pg.make("se", units=50, seed=41)
        _both(pkg, c, o, pes, id0, _dress(r2, False), [np.zeros(0, dtype=kswlib.ALNREG)] * len(r2), "no region at all")
    finally:
        c.close()


@pytest.mark.parametrize("n_w", [2, 1])
def test_no_record_in_the_main_round(pkg, n_w):
    """wantgen.long_fixes' regions alone: every wanted region is the host's after round 0, so the main round has no record and every
    record the text is made from is a patched one"""
    whole, c = _long_reference(pkg, 70, 20000)
    try:
        reads, vectors = [], []
        for rd, reg in wg.long_fixes(whole, 10000, score=300)[:n_w]:
            reg["seedcov"] = 60
            reads.append(rd), vectors.append(np.array([reg], dtype=kswlib.ALNREG))
        (_, _, a, res), st = _both(pkg, c, pg.opt(), None, 50, _dress(reads, False), vectors, f"{n_w} long fixes alone")
        assert (st["wanted"], st["fixed"], st["redone"], st["waits"], st["fallbacks"]) == (n_w, n_w, n_w, 6, 0), st
    finally:
        c.close()


# ---------------------------------------------------------------- the redo path where it grows and branches (tests/redogen.py)

def _past_the_slots(res):
    return (res["md_len"] > redogen.MD_SLOT) | (res["n_cigar"] > redogen.CIGAR_SLOT)


def test_the_overflow_area_outgrows_the_block(pkg):
    """The redone regions' records, CIGAR words and MD bytes go behind pass B's block in d_wanted.  A fresh context's block has under a
    MiB to spare; redogen.FIRST's 32 long reads need 1.6 MB there, so the live session moves the block under its own pointers
    (ensure_keep): seven waits.  The same slice again fits: six.  Then, on the block that has just been replaced, an ordinary slice with
    its regions and the 24-read slice with eight redone regions; then redogen.SECOND, whose 7.5 MB pass twice the capacity the first
    growth left, so that ensure_keep's max(bytes, 2 * capacity) has taken either side; and that slice again.  Every call byte for byte
    the host composition's text, with no fall-back.  That each slice does reach its branch is asserted on the yardstick's own records
    before the device call is trusted with it (and, from the substitutions alone, in tests/test_redogen_cpu.py).
    Measured on an MI355X: 1 662 733 bytes of overflow against 1 048 576, then 7 551 075 against 6 291 456; 1.3 s for the whole test."""
    whole, contigs = redogen.growth_reference()
    l_pac = len(whole)
    c = _context(pkg, contigs, wg.pack(whole), l_pac)
    try:
        o, caps = pg.opt(), []
        for spec, name in ((redogen.FIRST, "first"), (redogen.SECOND, "second")):
            reads, vectors, info = redogen.growth(whole, spec)
            seqs = _dress(reads, False)
            host = _host(pkg, c, o, None, 50, seqs, vectors)
            over, m = redogen.overflow_bytes(host[3]["md_len"], host[3]["n_cigar"])
            lb = redogen.lb_max(len(reads), sum(map(len, vectors)))
            if not caps:  # a fresh block: whatever its layout, it holds no more than this
                bound = redogen.first_cap(lb)
                caps.append(redogen.grown_cap(bound, lb + over + 4 * 64)[0])  # (... and no more than this once it has grown)
            else:
                bound = 2 * caps[0]
            print(f"{name} growth: {over} bytes of overflow in {m} regions against {bound}, predicted {redogen.predicted_overflow(info)}")
            assert m == info["n_long"] and over > bound, (name, over, bound, m)
            for what, waits in (("grows the block", 7), ("fits", 6)):
                _, st = _both(pkg, c, o, None, 50, seqs, vectors, f"{name} growth slice, {what}", host=host, expect_waits=waits)
                assert (st["redone"], st["fixed"], st["wanted"]) == (m, 0, len(reads)), (name, what, st)
            if name == "first":
                o2, pes2, id2, r2, v2 = pg.make("se", units=50, seed=41)
                _, st = _both(pkg, c, o2, pes2, id2, _dress(r2, False), v2, "an ordinary slice on the block that moved")
                assert st["wanted"] >= 30 and (st["redone"], st["waits"]) == (0, 4), st
                r3, v3, special = _outgrowing(whole, np.random.default_rng(61), l_pac)
                _, st = _both(pkg, c, o, None, 50, _dress(r3, False), v3, "eight redone regions on the block that moved")
                assert len(special) == 8 and (st["redone"], st["waits"], st["wanted"], st["fixed"]) == (8, 6, 32, 0), st
    finally:
        c.close()


@pytest.mark.parametrize("m", [255, 256, 257, 513])
def test_redone_counts_around_a_block(pkg, ctx, ref, m):
    """phase2_text_bind_kernel appends the host's regions to its list through an atomic counter and phase2_text_patch_kernel writes their
    records back, both in blocks of 256 lanes: one short of a block, a block, one more, two blocks and one.  The redone regions lie at
    irregular places in want order, on both strands, some by their MD and some by their CIGAR, some behind the sort."""
    reads, vectors = redogen.counted_slice(ref[0], m, seed=90)
    o, seqs = pg.opt(), _dress(reads, False)
    host = _host(pkg, ctx, o, None, 120, seqs, vectors)
    # Whether the overflow area fits behind the block depends on what the shared context has served before (513 regions outgrow a block
    # of one MiB): the first call may grow it, the second finds it large enough whatever came before
    dt, doff = ctx.phase2_text_device(o, ctx.idx, ctx.pac, None, 120, seqs, vectors, RG)
    _same_text(dt, doff, host[0], host[1], f"{m} redone regions, the block as it was")
    st = ctx.last_phase2_text_stats()
    assert st["redone"] == m and st["waits"] in (6, 7), st
    (_, _, a, res), st = _both(pkg, ctx, o, None, 120, seqs, vectors, f"{m} redone regions", host=host)
    past = _past_the_slots(res)
    j = np.flatnonzero(past)
    gaps = np.diff(j)
    assert int((gaps == 1).sum()) >= 20 and int((gaps > 1).sum()) >= 20 and len(set(gaps.tolist())) >= 4  # runs and single ones
    assert int((res["n_cigar"] > redogen.CIGAR_SLOT).sum()) >= m // 8 and int((res["md_len"] > redogen.MD_SLOT).sum()) >= m // 2
    assert 0 < int((res["rb"][past] >= wg.L_PAC).sum()) < m
    assert len(j) == m and (st["redone"], st["fixed"], st["waits"]) == (m, 0, 6) and st["wanted"] > m + 100, (m, len(j), st)
    # the list, 112 bytes per region, and one more status: nothing else of passes A and B came down
    assert st["d2h_bytes"] <= st["text_bytes"] + 8 * (len(reads) + 1) + 256 + 112 * m + 32, st


def test_paired_end_with_redone_mates(pkg, ctx, ref):
    """samtext_size_kernel composes both reads of a pair in one lane, each from its own records: pairs of which the first mate's record
    is a patched one and the second's is not, the reverse, both, and a redone mate beside one without any region; 72 pairs, past one
    block of decide_kernel"""
    reads, vectors, kinds = redogen.paired_slice(ref[0], 72, seed=95)
    assert set(kinds) == set(redogen.PAIR_KINDS) and len(reads) == 144
    o, pes = pg.opt(100, pg.PE), pg.pes_fr()
    (_, _, a, res), st = _both(pkg, ctx, o, pes, 7000, _dress(reads, True), vectors, "pairs with redone mates")
    expect = sum(k.count("redone") + k.count("cigar") for k in kinds)
    past = int(_past_the_slots(res).sum())
    assert past == expect and (st["redone"], st["waits"], st["fixed"]) == (past, 6, 0) and st["wanted"] > past, (past, expect, st)
    assert int((a["pd"]["paired"] != 0).sum()) >= 20  # (proper pairs among them, so the mates' records meet in one line's fields)


# ---------------------------------------------------------------- one session, in numbers

def test_one_upload_four_waits_and_only_text_down(pkg, ref):
    o, pes, id0, reads, vectors = pg.make("pe", n_wanted=1500)
    seqs = _dress(reads, True)
    total, n = sum(len(v) for v in vectors), len(reads)
    pool_bytes = len(sg.pack_reads(seqs)[1])
    assert total * 64 > 64 << 10 and pool_bytes > sum(len(r) for r in reads)
    # test_one_upload_and_three_waits' bound with the reads' bytes replaced by the per-read pool's, plus poff, the header and rg_id
    bound = total * 64 + pool_bytes + 16 * (n + 1) + 8 * pg.N_TERM + (8 << 10) + 8 * (n + 1) + 144 + len(RG)
    c = _context(pkg, wg.CONTIGS, ref[1], wg.L_PAC)
    try:
        host = _host(pkg, c, o, pes, id0, seqs, vectors)
        _, first = _both(pkg, c, o, pes, id0, seqs, vectors, "the call that makes the log table", host=host)
        _, again = _both(pkg, c, o, pes, id0, seqs, vectors, "the next call", host=host)
        for st, log_bytes in ((first, 8 << 17), (again, 0)):
            assert (st["waits"], st["sessions"], st["redone"]) == (4, 1, 0), st
            # the regions and the bases once: a second upload of either breaks the bound
            assert total * 64 + pool_bytes < st["h2d_bytes"] <= bound + log_bytes, (st, bound)
            # the text, its offsets and three status records: nothing of pass A or pass B
            assert st["text_bytes"] < st["d2h_bytes"] <= st["text_bytes"] + 8 * (n + 1) + 256, st
        assert first["h2d_bytes"] - again["h2d_bytes"] == 8 << 17
        assert all(again[k] == -1 for k in ("decide_ms", "wanted_ms", "gather_ms", "size_ms", "emit_ms"))
        # the same slice as two sessions on the same context: the records, slots and regions cross twice there
        dev = c.phase2_device(o, c.idx, c.pac, pes, id0, reads, vectors)
        p2 = c.last_phase2_stats()
        text, off = c.sam_text_batch(o, c.idx, pes, seqs, dev["regs"], dev, dev["res"], dev["cig"], dev["md"], RG, device=True)
        sx = c.last_samtext_stats()
        _same_text(text, off, host[0], host[1], "two sessions")
        assert (p2["waits"], sx["waits"]) == (3, 2)  # (and they still count as they did)
        assert again["h2d_bytes"] + again["d2h_bytes"] < p2["h2d_bytes"] + p2["d2h_bytes"] + sx["h2d_bytes"] + sx["d2h_bytes"], (again, p2, sx)
        c.set_kernel_timing(True)
        _, timed = _both(pkg, c, o, pes, id0, seqs, vectors, "timed", host=host)
        assert all(timed[k] > 0 for k in ("decide_ms", "wanted_ms", "gather_ms", "size_ms", "emit_ms")), timed
    finally:
        c.close()


def test_a_larger_slice_second_and_no_read(pkg, ref):
    """the text buffer, the blocks and the staging grow on a context that has served a small slice; n == 0 runs nothing"""
    c = _context(pkg, wg.CONTIGS, ref[1], wg.L_PAC)
    try:
        text, off = c.phase2_text_device(pg.opt(), c.idx, c.pac, None, 10, [], [], b"")
        st = c.last_phase2_text_stats()
        assert text == b"" and off.tolist() == [0]
        assert (st["units"], st["wanted"], st["reads"], st["sessions"], st["waits"], st["h2d_bytes"], st["d2h_bytes"]) == (0, 0, 0, 0, 0, 0, 0), st
        for mode, n_wanted in (("pe-all", 40), ("se-all", 4000), ("pe-all", 40)):
            o, pes, id0, reads, vectors = pg.make(mode, n_wanted=n_wanted, seed=6)
            (ht, _, _, _), _ = _both(pkg, c, o, pes, id0, _dress(reads, mode.startswith("pe")), vectors, f"{mode} {n_wanted}")
            assert n_wanted < 4000 or len(ht) > 1 << 20  # (past the buffers' first megabyte)
    finally:
        c.close()


# ---------------------------------------------------------------- refusals: all or nothing

def _refused(pkg, c, o, pes, seqs, vectors, code, what, idx=None, pac=None, text=True, text_off=True):
    """the call fails with `code`; text and text_off keep their sentinels and the vectors are the input's"""
    vecs = [np.ascontiguousarray(v, dtype=kswlib.ALNREG).reshape(-1).copy() for v in vectors]
    before = [v.tobytes() for v in vecs]
    out = sg.sentinels(len(seqs))
    lib = pkg.lib()
    if text and text_off:
        with pytest.raises(pkg.BmhError) as e:
            c.phase2_text_device(o, idx if idx is not None else c.idx, pac if pac is not None else c.pac, pes, 40, seqs, vecs, RG, out=out)
        rc = e.value.code
    else:  # a NULL output: past the binding
        oo = np.array(o, dtype=pkg.SAM_OPT).reshape(1)
        rc = lib.bmh_phase2_text_device(c._h, oo.ctypes.data_as(C.c_void_p), C.byref(c.idx), c.pac.ctypes.data_as(C.c_void_p), None, C.c_int64(40), 0, None, None,
                                        RG, C.cast(C.byref(out["text"]), C.c_void_p) if text else None,
                                        out["text_off"].ctypes.data_as(C.c_void_p) if text_off else None)
    assert rc == code, (what, rc)
    assert out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all(), what
    assert [v.tobytes() for v in vecs] == before, what


def _ordinary(pkg, c, seed=41):
    """the context is as good as before"""
    o, pes, id0, reads, vectors = pg.make("se", units=50, seed=seed)
    _both(pkg, c, o, pes, id0, _dress(reads, False), vectors, "after a refused call")


@pytest.mark.parametrize("mode", ["se-all", "pe"])
def test_refusals_before_the_upload(pkg, ctx, mode):
    o, pes, id0, reads, vectors = pg.make(mode, units=20, seed=3)
    pe = mode == "pe"
    seqs = _dress(reads, pe)
    sl = dict(opt=o, pes=pes, seqs=seqs, vectors=vectors, rg_id=RG, res=np.zeros(1, dtype=pkg.WANTED_RES), cig=None, md=None,
              dec=dict(pd=None, reg_mapq=None, n_want=np.ones(len(seqs), dtype=np.int32), want_k=np.zeros(sum(map(len, vectors)), dtype=np.int32)))
    applies = {"a read without a name", "mates with different names", "no pes", "an odd number of reads"}
    seen = set()
    for what, bad in sg.refusals(sl):  # what bmh_sam_text_batch refuses of the arguments this call has
        if what in applies:
            _refused(pkg, ctx, bad["opt"], bad["pes"], bad["seqs"], bad["vectors"], E_ARG, what)
            seen.add(what)
    assert seen == (applies if pe else {"a read without a name"})
    _refused(pkg, ctx, o, pes, seqs, vectors, E_ARG, "no text", text=False)
    _refused(pkg, ctx, o, pes, seqs, vectors, E_ARG, "no text_off", text_off=False)
    if pe:  # a window the pair table cannot hold: before any upload, and counted
        _refused(pkg, ctx, o, dg.special_pes("wide"), seqs, vectors, E_RANGE, "tables past their limit")
        st = ctx.last_phase2_text_stats()
        assert (st["fallbacks"], st["sessions"], st["h2d_bytes"], st["waits"]) == (1, 0, 0, 0), st
    _ordinary(pkg, ctx)


@pytest.mark.parametrize("which", ["lost", "bridge"])
def test_a_region_the_reference_aborts_on_fails_the_whole_call(pkg, ctx, ref, which):
    whole = ref[0]
    rd, reg = wg.lost_region(whole) if which == "lost" else wg.bridging_region(whole)
    o, pes, id0, reads, vectors = pg.make("se", units=30, seed=12)
    reads.insert(11, rd), vectors.insert(11, np.array([reg], dtype=kswlib.ALNREG))
    assert list(pkg.decide_batch(o, wg.L_PAC, None, 40, vectors)["want"][11]) == [0]
    _refused(pkg, ctx, o, pes, _dress(reads, False), vectors, E_ARG, which)
    assert ctx.last_phase2_text_stats()["fallbacks"] == 0
    _ordinary(pkg, ctx)


def test_a_wanted_window_past_65535_is_out_of_range(pkg):
    whole, c = _long_reference(pkg, 42, 80000)
    try:
        rd = whole[100:250].copy()
        a = wg.region(0, 150, 100, 100 + 65536, 150, 100, 150)
        b = wg.region(0, 150, 100, 250, 150, 100, 150)
        for x in (a, b):
            x["seedcov"] = 100
        o, seqs = pg.opt(), _dress([rd], False)
        _refused(pkg, c, o, None, seqs, [np.array([a], dtype=kswlib.ALNREG)], E_RANGE, "window")
        assert c.last_phase2_text_stats()["fallbacks"] == 0  # a kernel's refusal, not the tables'
        _both(pkg, c, o, None, 40, seqs, [np.array([b], dtype=kswlib.ALNREG)], "the same read with a window that fits")
        a["score"] = pg.T - 1  # unwanted, the long window is no obstacle
        _both(pkg, c, o, None, 40, seqs, [np.array([a], dtype=kswlib.ALNREG)], "unwanted")
    finally:
        c.close()


def test_refusals_without_the_resident_tables(pkg, ref):
    o, pes, id0, reads, vectors = pg.make("se", units=10, seed=43)
    seqs = _dress(reads, False)
    all_three = ("set_pac", "set_refidx", "set_refnames")
    for missing in all_three:
        c = _context(pkg, wg.CONTIGS, None, wg.L_PAC, tables=())
        try:
            c.pac = np.ascontiguousarray(ref[1], dtype=np.uint8)
            for f in all_three:
                if f == missing:
                    continue
                if f == "set_pac":
                    c.pac = c.set_pac(ref[1], wg.L_PAC)
                else:
                    getattr(c, f)(c.idx)
            _refused(pkg, c, o, pes, seqs, vectors, E_ARG, "without " + missing)
            if missing == "set_pac":
                c.pac = c.set_pac(ref[1], wg.L_PAC)
            else:
                getattr(c, missing)(c.idx)
            _both(pkg, c, o, pes, id0, seqs, vectors, "all resident after " + missing)
        finally:
            c.close()
    raw = _context(pkg, wg.CONTIGS, ref[1], wg.L_PAC, params=False)  # no parameters
    try:
        _refused(pkg, raw, o, pes, seqs, vectors, E_ARG, "no parameters")
    finally:
        raw.close()


# ---------------------------------------------------------------- the switch behind bmh_sam_batch

def _sam_batch(pkg, c, o, pes, id0, vecs, reads, rg_id=b"", dress=None):
    """bmh_sam_batch over a slice: (per read its SAM text, the vectors as the call left them).  dress: per read (name, comment or
    None, qualities or None); without it the names, comments and qualities these tests make up."""
    lib = pkg.lib()
    lib.bmh_sam_batch.restype = C.c_int
    pe = _is_pe(o)
    seqs = (pkg._Seq * max(len(reads), 1))()
    keep = []
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        keep.append(r)
        name, comment, qual = dress[i] if dress is not None else (b"r%d" % (i // 2 if pe else i), b"co" if i % 3 == 0 else None, bytes([35 + i % 40]) * len(r) if i % 4 else None)
        seqs[i] = pkg._Seq(len(r), name, comment, r.ctypes.data, qual, None)
    bufs = [np.array(v, dtype=kswlib.ALNREG, copy=True) for v in vecs]
    c_regs = (kswlib.CAlnregV * max(len(bufs), 1))()
    for i, a in enumerate(bufs):
        c_regs[i].n = c_regs[i].m = len(a)
        c_regs[i].a = a.ctypes.data if len(a) else None
    rc = lib.bmh_sam_batch(c._h, o.ctypes.data_as(C.c_void_p), C.byref(c.idx), c.pac.ctypes.data_as(C.c_void_p),
                           pes.ctypes.data_as(C.c_void_p) if pes is not None else None, C.c_int64(id0), len(reads), seqs, c_regs, rg_id)
    assert rc == 0, (rc, lib.bmh_last_error(c._h))
    text = []
    for s in seqs[:len(reads)]:
        text.append(C.string_at(s.sam))
        pkg._libc.free(C.c_void_p(s.sam))
    return text, [a.tobytes() for a in bufs]


@pytest.mark.parametrize("mode", ["se", "pe"])
def test_switch_behind_sam_batch(pkg, ref, mode):
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=400, seed=31)
    rng = np.random.default_rng(32)
    for name, rd, reg, expect in wg.overhangs(ref[0])[:6]:  # some regions to fix, behind the sort
        b, v = _behind(rng, ref[0], rd, reg)
        reads += [b, kswgen.rand_seq(rng, 60)] if mode == "pe" else [b]
        vectors += [v, np.zeros(0, dtype=kswlib.ALNREG)] if mode == "pe" else [v]
    came = [np.array(v, dtype=kswlib.ALNREG, copy=True).tobytes() for v in vectors]
    c = _context(pkg, wg.CONTIGS, ref[1], wg.L_PAC)
    try:
        t0, r0 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert r0 != came  # the default route leaves the vectors sorted and marked
        assert c.last_phase2_text_stats()["sessions"] == -1  # nothing fused yet
        c.set_phase2_text_device(True)
        t1, r1 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t1 and r1 == came  # the same text; the vectors as they came
        st = c.last_phase2_text_stats()
        mapped = sum(1 for t in t0 for l in t.splitlines() if not int(l.split(b"\t")[1]) & 4)
        assert (st["reads"], st["lines"], st["text_bytes"]) == (len(reads), sum(t.count(b"\n") for t in t0), sum(map(len, t0))), st
        assert st["wanted"] == mapped and st["fixed"] >= 4 and (st["sessions"], st["waits"], st["fallbacks"]) == (1, 4, 0), (st, mapped)
        # the other switches do not matter while this one is on, and their statistics are not this route's
        c.set_phase2_device(True), c.set_samtext_device(True)
        t2, r2 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t2 and r2 == came and c.last_phase2_stats()["sessions"] == 0 and c.last_samtext_stats()["reads"] == 0
        c.set_phase2_device(False), c.set_samtext_device(False)
        # a call that returns before its passes leaves its own statistics, not the previous slice's
        assert _sam_batch(pkg, c, o, pes, id0, [], []) == ([], [])
        st = c.last_phase2_text_stats()
        assert (st["units"], st["reads"], st["sessions"], st["h2d_bytes"], st["waits"], st["size_ms"]) == (0, 0, 0, 0, 0, -1), st
        if mode == "pe":  # a window the pair table cannot hold: the slice goes down the existing route, whatever the other switches say
            wide = dg.special_pes("wide")
            c.set_phase2_text_device(False)
            t3, r3 = _sam_batch(pkg, c, o, wide, id0, vectors, reads, b"grp")
            for two in (False, True):
                c.set_phase2_text_device(True), c.set_phase2_device(two), c.set_samtext_device(two)
                t4, r4 = _sam_batch(pkg, c, o, wide, id0, vectors, reads, b"grp")
                assert t3 == t4 and r3 == r4
                st = c.last_phase2_text_stats()
                assert (st["fallbacks"], st["sessions"], st["h2d_bytes"]) == (1, 0, 0), st
            c.set_phase2_device(False), c.set_samtext_device(False)
        # off again: nothing fused, the statistics stay
        c.set_phase2_text_device(False)
        before = c.last_phase2_text_stats()
        t5, r5 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t5 and r0 == r5 and c.last_phase2_text_stats() == before
    finally:
        c.close()


def test_switch_behind_sam_batch_with_redone_regions(pkg):
    """bmh_phase2_text_routed_ with regions to redo: the session leaves its gate around the host's redo and takes it again, inside
    bmh_sam_batch, and the caller's vectors still come back as they came"""
    whole, c = _long_reference(pkg, 60, 20000)
    try:
        reads, vectors, special = _outgrowing(whole, np.random.default_rng(61))
        plain = [k for k in range(len(reads)) if k not in special]
        pr, pv = [reads[k] for k in plain], [vectors[k] for k in plain]
        came = [np.array(v, dtype=kswlib.ALNREG, copy=True).tobytes() for v in vectors]
        o = pg.opt()
        t0, r0 = _sam_batch(pkg, c, o, None, 50, vectors, reads, b"grp")
        p0, q0 = _sam_batch(pkg, c, o, None, 90, pv, pr, b"grp")
        assert r0 != came and c.last_phase2_text_stats()["sessions"] == -1  # the default route sorts and marks; nothing fused yet
        c.set_phase2_text_device(True)
        t1, r1 = _sam_batch(pkg, c, o, None, 50, vectors, reads, b"grp")
        assert t0 == t1 and r1 == came  # the same text; the vectors as they came
        st = c.last_phase2_text_stats()
        assert len(special) == 8 and (st["redone"], st["waits"], st["fallbacks"], st["sessions"], st["wanted"], st["fixed"]) == (8, 6, 0, 1, 32, 0), st
        assert (st["reads"], st["lines"], st["text_bytes"]) == (len(reads), sum(t.count(b"\n") for t in t0), sum(map(len, t0))), st
        # the next slice on the same context is an ordinary one again
        p1, q1 = _sam_batch(pkg, c, o, None, 90, pv, pr, b"grp")
        assert p0 == p1 and q1 == [np.array(v, dtype=kswlib.ALNREG, copy=True).tobytes() for v in pv]
        st = c.last_phase2_text_stats()
        assert (st["redone"], st["waits"], st["fallbacks"], st["sessions"], st["wanted"]) == (0, 4, 0, 1, len(pr)), st
        c.set_phase2_text_device(False)
        t2, r2 = _sam_batch(pkg, c, o, None, 50, vectors, reads, b"grp")
        assert t0 == t2 and r0 == r2
    finally:
        c.close()
