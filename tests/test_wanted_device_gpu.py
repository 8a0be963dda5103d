"""bmh_wanted_cigar_device (csrc/wanted.hip: the planning kernels over host/regplan_core.h, then the region kernels) against
bmh_wanted_cigar_batch, the host form over the gcc build of the same text: the record array and both pools byte for byte.  Then the
committed fixture of the compiled reference through the device form, regions that hang over the end of a reference sequence, a
12 000-base query, alignments that outgrow the device's slots, vectors the kernels must refuse, and the switch behind bmh_sam_batch."""
import ctypes as C

import numpy as np
import pytest

import decidegen as dg
import kswgen
import kswlib
import postgen
import regplan as rp
import wantgen as wg
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -3, -4


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ref():
    whole, pac = wg.reference()
    return whole, pac


@pytest.fixture(scope="module")
def ctx(pkg, ref):
    c = pkg.Context(0, kswlib.make_params())
    c.idx = pkg.make_refidx(wg.CONTIGS)
    c.pac = c.set_pac(ref[1], wg.L_PAC)
    c.set_refidx(c.idx)
    yield c
    c.close()


def _used(res):
    return int(res["n_cigar"].sum()), int((res["md_len"].astype(np.int64) + 1).sum())


def _same(dev, host, what):
    (dr, dc, dm), (hr, hc, hm) = dev, host
    assert len(dr) == len(hr), what
    bad = [j for j in range(len(hr)) if dr[j].tobytes() != hr[j].tobytes()]
    assert not bad, (what, len(bad), bad[:5], dr[bad[0]], hr[bad[0]])
    cu, mu = _used(hr)
    assert np.array_equal(dc[:cu], hc[:cu]) and bytes(dm[:mu]) == bytes(hm[:mu]), what


def _both(ctx, w, reads, vectors, want, what, idx=None, pac=None):
    idx, pac = idx if idx is not None else ctx.idx, pac if pac is not None else ctx.pac
    host = ctx.wanted_cigar_batch(idx, pac, w, reads, vectors, want)
    dev = ctx.wanted_cigar_batch(idx, pac, w, reads, vectors, want, device=True)
    _same(dev, host, what)
    return host


def _kinds(res):
    """how many records are {no-gap, 1 try, 2 tries, 3 tries, with tries sharing a task}"""
    b, t = res["band"], res["tries"]
    nogap = b[:, 0] == -1
    shared = ~nogap & (((b[:, 1] == b[:, 0]) & (b[:, 1] >= 0)) | ((b[:, 2] == b[:, 1]) & (b[:, 2] >= 0)))
    return [int(nogap.sum())] + [int((~nogap & (t == k)).sum()) for k in (1, 2, 3)] + [int(shared.sum())]


@pytest.mark.parametrize("w", [100, 5])
@pytest.mark.parametrize("n_wanted", [1, 63, 64, 65, 257, 1025, 1500])
def test_sizes(ctx, ref, n_wanted, w):
    """one, around a wave, one more than the planning kernels' 256-lane blocks and than the scan's 1024 lanes, several blocks"""
    rng = np.random.default_rng(1000 + n_wanted)
    reads, vectors, want = wg.slice_of(rng, ref[0], n_wanted)
    assert sum(len(k) for k in want) == n_wanted and want[0] and want[-1]
    ctx.set_params(kswlib.make_params(w=w))
    try:
        host = _both(ctx, w, reads, vectors, want, f"{n_wanted} wanted, w={w}")
        assert ctx.last_wanted_stats()[:3] == (n_wanted, 0, 0)
        assert not (host[0]["flags"] != 0).any()
        if n_wanted >= 1025:
            assert any(len(k) == 0 for k in want[1:-1]) and max(len(k) for k in want) == 6
            kinds = _kinds(host[0])
            assert min(kinds) >= 16, kinds
    finally:
        ctx.set_params(kswlib.make_params())


def test_planning_kernels_time_in_timing_mode(ctx, ref):
    """the stand-alone call's kernel time: -1 with timing off, positive with it on, -1 again once it is off; records and pools as the host's"""
    reads, vectors, want = wg.slice_of(np.random.default_rng(65), ref[0], 65)
    _both(ctx, 100, reads, vectors, want, "timing off")
    assert ctx.last_wanted_stats() == (65, 0, 0, -1)
    ctx.set_kernel_timing(True)
    try:
        _both(ctx, 100, reads, vectors, want, "timing on")
        wanted, fixed, redone, ms = ctx.last_wanted_stats()
        assert (wanted, fixed, redone) == (65, 0, 0) and ms > 0, ms
    finally:
        ctx.set_kernel_timing(False)
    _both(ctx, 100, reads, vectors, want, "timing off again")
    assert ctx.last_wanted_stats() == (65, 0, 0, -1)


def test_no_want_at_all(ctx, ref):
    rng = np.random.default_rng(3)
    reads, vectors, _ = wg.random_slice(rng, ref[0], 20)
    sentinel = (np.full(4, 0x5a, dtype=np.uint8).view(np.uint8), np.full(8, 0xa5a5a5a5, dtype=np.uint32), np.full(8, 0x5a, dtype=np.uint8))
    out = (np.zeros(0, dtype=load_package().WANTED_RES), sentinel[1].copy(), sentinel[2].copy())
    res, cig, md = ctx.wanted_cigar_batch(ctx.idx, ctx.pac, 100, reads, vectors, [[] for _ in reads], device=True, out=out)
    assert len(res) == 0 and (cig == sentinel[1]).all() and (md == sentinel[2]).all()
    assert ctx.last_wanted_stats()[:3] == (0, 0, 0)


def test_reference_fixture_through_the_device_form(pkg):
    """cigar_golden.npz: CIGAR, NM and MD of the compiled reference's mem_reg2aln, each request as the one wanted region of its read"""
    n = 0
    c = pkg.Context(0, kswlib.make_params())
    try:
        for p, l_pac, pac, reads, reqs, exp in kswlib.golden_cigar_groups():
            c.set_params(p)
            pac = c.set_pac(pac, l_pac)
            idx = pkg.make_refidx([(0, l_pac)])
            c.set_refidx(idx)
            rr, vv = [], []
            for rq in reqs:
                rr.append(reads[int(rq["read"])])
                vv.append(np.array([wg.region(rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"])], dtype=kswlib.ALNREG))
            res, cig, md = c.wanted_cigar_batch(idx, pac, int(p["w"]), rr, vv, [[0]] * len(rr), device=True)
            mdb = bytes(md)
            for rq, r, (en, ew, enm, emd), read in zip(reqs, res, exp, rr):
                assert (int(r["qb"]), int(r["qe"]), int(r["rb"]), int(r["re"])) == (int(rq["qb"]), int(rq["qe"]), int(rq["rb"]), int(rq["re"]))
                words = cig[int(r["cigar_off"]): int(r["cigar_off"]) + int(r["n_cigar"])]
                fw, fmd = kswlib.finish_aln(words, mdb[int(r["md_off"]): int(r["md_off"]) + int(r["md_len"])], rq, len(read), l_pac)
                assert len(fw) == en and np.array_equal(fw, ew), f"req {rq}: gpu={fw} ref={ew}"
                assert int(r["NM"]) == enm and fmd == emd
                n += 1
    finally:
        c.close()
    assert n >= 2000


def test_overhanging_regions(ctx, ref):
    whole = ref[0]
    cases = wg.overhangs(whole)
    rng = np.random.default_rng(8)
    fill_r, fill_v, fill_w = wg.random_slice(rng, whole, 40)  # ordinary reads around them
    reads = fill_r[:20] + [c[1] for c in cases] + fill_r[20:]
    vectors = fill_v[:20] + [np.array([c[2]], dtype=kswlib.ALNREG) for c in cases] + fill_v[20:]
    want = fill_w[:20] + [[0]] * len(cases) + fill_w[20:]
    host = _both(ctx, 100, reads, vectors, want, "overhangs")
    first = sum(len(k) for k in fill_w[:20])
    recs = host[0][first:first + len(cases)]
    n_fix = sum(c[3] != "none" for c in cases)
    assert n_fix >= 32 and ctx.last_wanted_stats()[:3] == (len(host[0]), n_fix, 0)
    p = kswlib.make_params()
    seen = {k: 0 for k in ("Mb", "Me", "Db", "De", "none")}
    for (name, rd, reg, expect), r in zip(cases, recs):
        moved = bool(int(r["flags"]) & 4)
        rb, re = int(reg["rb"]), int(reg["re"])
        v, cb, ce = rp.xref_test(wg.CONTIGS, wg.L_PAC, rb, re)
        assert v == int(moved) and moved == (expect != "none"), name
        got = (int(r["qb"]), int(r["qe"]), int(r["rb"]), int(r["re"]))
        if not moved:
            assert got == (0, len(rd), rb, re), name
            seen["none"] += 1
            continue
        # bwa_fix_xref2's one alignment on the CPU oracle (a score estimate low enough infers more than opt->w, so the band is the
        # region's 100 and one try is enough), then the walk of bwa.c:199-221 as tests/regplan.py restates it
        rq = np.zeros((), kswlib.CIGAR_REQ)
        rq["qb"], rq["qe"], rq["rb"], rq["re"], rq["truesc"], rq["reg_w"] = 0, len(rd), rb, re, -100000, 100
        _, words, _, _, tries = kswlib.orc_reg2cigar(p, wg.L_PAC, ref[1], rd, rq)
        assert tries == 1, name
        verdict, *want = rp.xref_cut(words, cb, ce, 0, len(rd), rb, re)
        assert verdict == 0 and got == tuple(want), (name, got, want)
        took = rp.cut_branches(words, cb, ce, rb, re)
        assert len(took) == 1, (name, took)
        if name[-1] == "+":  # (a hit on the reverse strand is aligned backwards and its CIGAR walked forwards, as the reference does)
            assert took == {expect}, (name, took)
        seen[took.pop()] += 1
        assert int(r["NM"]) <= 6, (name, r)  # error-free reads: what is left aligns almost perfectly
    assert min(seen.values()) >= 4, seen


def _sentinels(pkg, n_w):
    return (np.frombuffer(b"\x5a" * (72 * n_w), dtype=pkg.WANTED_RES).copy(), np.full(400 * n_w + 64, 0xa5a5a5a5, dtype=np.uint32),
            np.full(1200 * n_w + 64, 0x5a, dtype=np.uint8))


def _refused(pkg, ctx, reads, vectors, want, code, device=True, idx=None, pac=None):
    n_w = sum(len(k) for k in want)
    out = _sentinels(pkg, n_w)
    keep = [a.copy() for a in out]
    with pytest.raises(pkg.BmhError) as e:
        ctx.wanted_cigar_batch(idx if idx is not None else ctx.idx, pac if pac is not None else ctx.pac, 100, reads, vectors, want, device=device, out=out)
    assert e.value.code == code, e.value
    for a, b in zip(out, keep):
        assert a.tobytes() == b.tobytes()  # a refused call leaves the outputs untouched


@pytest.mark.parametrize("which", ["lost", "bridge"])
def test_a_region_the_reference_aborts_on_fails_the_whole_call(pkg, ctx, ref, which):
    whole = ref[0]
    rd, reg = wg.lost_region(whole) if which == "lost" else wg.bridging_region(whole)
    rng = np.random.default_rng(12)
    reads, vectors, want = wg.random_slice(rng, whole, 30)
    reads.insert(11, rd), vectors.insert(11, np.array([reg], dtype=kswlib.ALNREG)), want.insert(11, [0])
    _refused(pkg, ctx, reads, vectors, want, E_ARG, device=False)
    _refused(pkg, ctx, reads, vectors, want, E_ARG, device=True)
    del reads[11], vectors[11], want[11]
    _both(ctx, 100, reads, vectors, want, "the same slice without it")


def _bad_slice(ref, which):
    rng = np.random.default_rng(40)
    reads, vectors, want = wg.random_slice(rng, ref[0], 70)
    i = next(i for i in range(30, 70) if len(want[i]) >= 1)
    k = want[i][0]
    v = vectors[i] = vectors[i].copy()
    if which == "want_k past the vector":
        want[i][0] = len(v)
    elif which == "want_k negative":
        want[i][0] = -1
    elif which == "qe past the read":
        v[k]["qe"] = len(reads[i]) + 1
    elif which == "qb negative":
        v[k]["qb"] = -3
    elif which == "rb negative":
        v[k]["rb"] = -5
    elif which == "re past the reference":
        v[k]["rb"], v[k]["re"] = 2 * wg.L_PAC - 20, 2 * wg.L_PAC + 1
    elif which == "empty window":
        v[k]["re"] = v[k]["rb"]
    elif which == "huge window":
        v[k]["rb"], v[k]["re"] = 10, 10 + (1 << 40)
    return reads, vectors, want


@pytest.mark.parametrize("which", ["want_k past the vector", "want_k negative", "qe past the read", "qb negative", "rb negative",
                                   "re past the reference", "empty window", "huge window"])
def test_invalid_vectors_are_refused_by_checks(pkg, ctx, ref, which):
    reads, vectors, want = _bad_slice(ref, which)
    _refused(pkg, ctx, reads, vectors, want, E_ARG)
    rng = np.random.default_rng(41)  # and the context is as good as before
    _both(ctx, 100, *wg.random_slice(rng, ref[0], 50), "after a refused call")


def test_a_window_past_65535_is_out_of_range(pkg):
    rng = np.random.default_rng(42)
    l_pac = 80000
    whole = kswgen.rand_seq(rng, l_pac)
    c = pkg.Context(0, kswlib.make_params())
    try:
        idx = pkg.make_refidx([(0, l_pac)])
        pac = c.set_pac(wg.pack(whole), l_pac)
        c.set_refidx(idx)
        rd = whole[100:250].copy()
        _refused(pkg, c, [rd], [np.array([wg.region(0, 150, 100, 100 + 65536, 150, 100)], dtype=kswlib.ALNREG)], [[0]], E_RANGE, idx=idx, pac=pac)
        _refused(pkg, c, [rd], [np.array([wg.region(0, 150, 100, 100 + 65536, 150, 100)], dtype=kswlib.ALNREG)], [[0]], E_RANGE, device=False, idx=idx, pac=pac)
    finally:
        c.close()


def test_refusals_without_the_resident_tables(pkg, ref):
    rng = np.random.default_rng(43)
    reads, vectors, want = wg.random_slice(rng, ref[0], 10)
    c = pkg.Context(0, kswlib.make_params())
    try:
        c.idx, c.pac = pkg.make_refidx(wg.CONTIGS), ref[1]
        _refused(pkg, c, reads, vectors, want, E_ARG)  # neither
        c.set_refidx(c.idx)
        _refused(pkg, c, reads, vectors, want, E_ARG)  # no reference
        c.pac = c.set_pac(ref[1], wg.L_PAC)
        _both(c, 100, reads, vectors, want, "both resident")
        c.set_refidx(None)
        _refused(pkg, c, reads, vectors, want, E_ARG)  # the table dropped
        c.set_refidx(pkg.make_refidx([(0, wg.L_PAC)]))
        _refused(pkg, c, reads, vectors, want, E_ARG)  # another reference's table
        # a table with other offsets but as many sequences and the same length replaces the resident one
        c.set_refidx(c.idx)
        cases = wg.overhangs(ref[0])
        rr, vv = [x[1] for x in cases], [np.array([x[2]], dtype=kswlib.ALNREG) for x in cases]
        a = _both(c, 100, rr, vv, [[0]] * len(cases), "the generator's table")
        other = pkg.make_refidx([(0, 2990), (2990, 1011), (4001, 507)])
        c.set_refidx(other)
        b = _both(c, 100, rr, vv, [[0]] * len(cases), "a table of the same shape", idx=other)
        assert (a[0]["rb"] != b[0]["rb"]).any() or (a[0]["re"] != b[0]["re"]).any()
    finally:
        c.close()


def _long_reference(pkg, seed, l_pac):
    whole = kswgen.rand_seq(np.random.default_rng(seed), l_pac)
    c = pkg.Context(0, kswlib.make_params())
    c.idx = pkg.make_refidx([(0, l_pac // 2), (l_pac // 2, l_pac - l_pac // 2)])
    c.pac = c.set_pac(wg.pack(whole), l_pac)
    c.set_refidx(c.idx)
    return whole, c


def test_a_region_of_12000_query_bases(pkg):
    """past the 10 176 query columns of the LDS kernel: the band ring of launch_global, so the status record's long-task shape is used"""
    whole, c = _long_reference(pkg, 50, 40000)
    try:
        rng = np.random.default_rng(51)
        rd = kswgen.mutate(rng, whole[3000:15000], sub=0.01, ins=0.001, dele=0.001)
        short = whole[30000:30150].copy()
        reads = [short, rd, wg.revcomp(rd), short]
        vectors = [np.array([wg.region(0, 150, 30000, 30150, 140, 100)], dtype=kswlib.ALNREG),
                   np.array([wg.region(0, len(rd), 3000, 15000, len(rd) - 300, 100)], dtype=kswlib.ALNREG),
                   np.array([wg.region(0, len(rd), 80000 - 15000, 80000 - 3000, len(rd) + 500, 100)], dtype=kswlib.ALNREG),
                   np.array([wg.region(0, 150, 30000, 30150, 150, 100)], dtype=kswlib.ALNREG)]
        host = _both(c, 100, reads, vectors, [[0]] * 4, "12 000 bases", idx=c.idx, pac=c.pac)
        assert len(rd) > 10176 and int(host[0]["n_cigar"][1]) > 24  # (and so it is redone on the host as well)
        assert c.last_wanted_stats()[2] == 2 and list(host[0]["flags"]) == [0, 8, 8, 0]
    finally:
        c.close()


def test_alignments_that_outgrow_the_slots_are_redone(pkg):
    """a substitution every 3 bases of 250: an MD past 96 bytes and past the 128 of its slot; 14 separated indels: a CIGAR past 24 words; the rest of the batch is not redone"""
    whole, c = _long_reference(pkg, 60, 20000)
    try:
        rng = np.random.default_rng(61)
        reads, vectors = [], []
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
            rb, re = (pos, pos + tl) if not rev else (40000 - pos - tl, 40000 - pos)
            reads.append(wg.revcomp(rd) if rev else rd)
            vectors.append(np.array([wg.region(0, len(rd), rb, re, len(rd) - 40, 100)], dtype=kswlib.ALNREG))
        host = _both(c, 100, reads, vectors, [[0]] * 24, "long MD and CIGAR", idx=c.idx, pac=c.pac)
        res = host[0]
        for k in range(24):
            redone = bool(int(res["flags"][k]) & 8)
            assert redone == (k % 6 in (2, 4)), (k, res[k])
            if k % 6 == 2:
                assert int(res["md_len"][k]) > 128
            if k % 6 == 4:
                assert int(res["n_cigar"][k]) > 24
        assert c.last_wanted_stats()[:3] == (24, 0, 8)
    finally:
        c.close()


def test_a_fix_whose_alignment_outgrows_its_slot_is_redone_with_its_fix(pkg):
    whole, c = _long_reference(pkg, 70, 20000)
    try:
        b = 10000
        parts, at = [], b - 300
        for j in range(14):  # 14 separated indels on the way to the boundary, then 60 bases past it
            parts.append(whole[at:at + 20])
            at += 20
            if j % 2:
                parts.append(np.array([(int(whole[at]) + 2) & 3, (int(whole[at]) + 1) & 3], dtype=np.uint8))
            else:
                at += 2
        parts.append(whole[at:b + 60])
        rd = np.concatenate(parts)
        plain = whole[b - 100:b + 30].copy()
        reads = [plain, rd, wg.revcomp(rd)]
        vectors = [np.array([wg.region(0, 130, b - 100, b + 30, 130, 100)], dtype=kswlib.ALNREG),
                   np.array([wg.region(0, len(rd), b - 300, b + 60, len(rd) - 50, 100)], dtype=kswlib.ALNREG),
                   np.array([wg.region(0, len(rd), 40000 - b - 60, 40000 - b + 300, len(rd) - 50, 100)], dtype=kswlib.ALNREG)]
        host = _both(c, 100, reads, vectors, [[0]] * 3, "a long fix", idx=c.idx, pac=c.pac)
        assert list(host[0]["flags"]) == [4, 12, 12] and int(host[0]["re"][1]) == b and int(host[0]["rb"][2]) == 40000 - b
        assert c.last_wanted_stats()[:3] == (3, 3, 2)
    finally:
        c.close()


@pytest.mark.parametrize("n_w", [2, 1])
def test_no_record_in_the_main_round(pkg, n_w):
    """the long fixes of the test above without the plain read: every wanted region is the host's after round 0, so the main round has
    no record, no slot comes down and every record is redone"""
    whole, c = _long_reference(pkg, 70, 20000)
    try:
        b = 10000
        pairs = wg.long_fixes(whole, b)[:n_w]
        reads, vectors = [rd for rd, _ in pairs], [np.array([reg], dtype=kswlib.ALNREG) for _, reg in pairs]
        host = _both(c, 100, reads, vectors, [[0]] * n_w, f"{n_w} long fixes alone", idx=c.idx, pac=c.pac)
        assert list(host[0]["flags"]) == [12] * n_w and int(host[0]["re"][0]) == b
        assert n_w < 2 or int(host[0]["rb"][1]) == 40000 - b
        assert c.last_wanted_stats()[:3] == (n_w, n_w, n_w)
    finally:
        c.close()


def test_a_want_list_that_skips_regions_out_of_vector_order(pkg):
    """want_k = [2, 0] of the second read's three regions, behind a read that wants none of its two; region 2 has an MD past its slot:
    the redo takes (read, k) from the want list and the region from the flat arena at roff[read] + k"""
    whole, c = _long_reference(pkg, 80, 20000)
    try:
        rng = np.random.default_rng(81)
        segs, regs = [], []
        for pos, ln in ((600, 150), (4100, 140), (7300, 150), (12500, 130), (15200, 250)):
            sg = kswgen.mutate(rng, whole[pos:pos + ln], sub=0.02)
            if ln == 250:  # a substitution every 3 bases: an MD past 128 bytes
                sg = whole[pos:pos + ln].copy()
                sg[::3] = (sg[::3] + 1) & 3
            segs.append(sg), regs.append((pos, ln))

        def vector(ks):
            q, out = 0, []
            for k in ks:
                pos, ln = regs[k]
                out.append(wg.region(q, q + len(segs[k]), pos, pos + ln, len(segs[k]) - 40, 100))
                q += len(segs[k])
            return np.concatenate([segs[k] for k in ks]), np.array(out, dtype=kswlib.ALNREG)

        (r0, v0), (r1, v1) = vector([0, 1]), vector([2, 3, 4])
        host = _both(c, 100, [r0, r1], [v0, v1], [[], [2, 0]], "want_k = [2, 0]", idx=c.idx, pac=c.pac)
        res = host[0]
        assert list(res["flags"]) == [8, 0] and int(res["md_len"][0]) > 128
        assert (int(res["qb"][0]), int(res["rb"][0])) == (int(v1[2]["qb"]), 15200) and (int(res["qb"][1]), int(res["rb"][1])) == (0, 7300)
        assert c.last_wanted_stats()[:3] == (2, 0, 1)
    finally:
        c.close()


# ---------------------------------------------------------------- the switch behind bmh_sam_batch

class _Seq(C.Structure):  # bmh_seq_t
    _fields_ = [("l_seq", C.c_int32), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


def _sam_batch(pkg, ctx, o, pes, id0, vecs, idx, pac, reads):
    lib = pkg.lib()
    lib.bmh_sam_batch.restype = C.c_int
    seqs = (_Seq * max(len(reads), 1))()
    keep = []
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        keep.append(r)
        seqs[i] = _Seq(len(r), b"r%d" % (i // 2 if int(o["flag"]) & dg.PE else i), None, r.ctypes.data, None, None)
    bufs = [np.array(v, dtype=kswlib.ALNREG, copy=True) for v in vecs]
    c_regs = (kswlib.CAlnregV * max(len(bufs), 1))()
    for i, a in enumerate(bufs):
        c_regs[i].n = c_regs[i].m = len(a)
        c_regs[i].a = a.ctypes.data if len(a) else None
    rc = lib.bmh_sam_batch(ctx._h, o.ctypes.data_as(C.c_void_p), C.byref(idx), pac.ctypes.data_as(C.c_void_p),
                           pes.ctypes.data_as(C.c_void_p) if pes is not None else None, C.c_int64(id0), len(reads), seqs, c_regs, b"")
    assert rc == 0, (rc, lib.bmh_last_error(ctx._h))
    text = []
    for s in seqs[:len(reads)]:
        text.append(C.string_at(s.sam))
        pkg._libc.free(C.c_void_p(s.sam))
    return text, [a.tobytes() for a in bufs]


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_switch_behind_sam_batch(pkg, paired):
    rng = np.random.default_rng(31)
    whole = kswgen.rand_seq(rng, dg.L_PAC)
    if paired:
        vecs = dg.pe_vectors(33, 300)
        o, pes = dg.pe_opt(0), dg.fixture_pes(0)
    else:
        vecs = postgen.region_vectors(rng, 400, dg.L_PAC)
        o, pes = dg.sam_opt(), None
    ok = [all(0 <= int(r["rb"]) and int(r["re"]) <= 2 * dg.L_PAC and not int(r["rb"]) < dg.L_PAC < int(r["re"]) for r in v) for v in vecs]
    if paired:
        ok = [a and b for a, b in zip(ok[::2], ok[1::2]) for _ in range(2)]
    vecs = [v for v, k in zip(vecs, ok) if k]
    assert len(vecs) > 300
    reads = [kswgen.rand_seq(rng, 150) for _ in vecs]
    half = dg.L_PAC // 2
    ctx = pkg.Context(0, kswlib.make_params())
    try:
        idx = pkg.make_refidx([(0, half), (half, dg.L_PAC - half)])
        pac = ctx.set_pac(wg.pack(whole), dg.L_PAC)
        ctx.set_refidx(idx)
        t0, r0 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, idx, pac, reads)
        n_lines = sum(len(t.splitlines()) for t in t0)
        ctx.set_wanted_device(True)
        t1, r1 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, idx, pac, reads)
        assert t0 == t1 and r0 == r1
        wanted, fixed, redone, _ = ctx.last_wanted_stats()
        mapped = sum(1 for t in t0 for l in t.splitlines() if not int(l.split(b"\t")[1]) & 4)
        assert wanted == mapped and 0 < wanted <= n_lines and 0 < redone <= wanted, (wanted, mapped, n_lines, redone)  # (random reads: long MDs)
        ctx.set_decide_device(True)  # both switches: pass A and pass B are both the device's, the text is the same
        t2, r2 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, idx, pac, reads)
        assert t0 == t2 and r0 == r2
        assert ctx.last_decide_stats()[:2] == (len(vecs) // 2 if paired else len(vecs), 0) and ctx.last_wanted_stats()[0] == wanted
        # a call that returns before its alignments leaves its own statistics, not the previous slice's
        assert _sam_batch(pkg, ctx, o, pes, 4000, [], idx, pac, []) == ([], []) and ctx.last_wanted_stats()[:3] == (0, 0, 0)
        if paired:  # a window the pair table cannot hold: host decisions, then the device form
            wide = dg.special_pes("wide")
            ctx.set_decide_device(False), ctx.set_wanted_device(False)
            t3, r3 = _sam_batch(pkg, ctx, o, wide, 4000, vecs, idx, pac, reads)
            ctx.set_decide_device(True), ctx.set_wanted_device(True)
            t4, r4 = _sam_batch(pkg, ctx, o, wide, 4000, vecs, idx, pac, reads)
            assert t3 == t4 and r3 == r4
            assert ctx.last_decide_stats()[:2] == (0, 1) and ctx.last_wanted_stats()[0] > 0
    finally:
        ctx.close()
