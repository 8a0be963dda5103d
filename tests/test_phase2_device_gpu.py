"""bmh_phase2_device -- pass A (decide_kernel) and pass B (the planning kernels, the region kernels, wanted_result_kernel) as one
device session -- against the host composition bmh_decide_batch, then bmh_wanted_cigar_batch: the vectors, the pair verdicts,
reg_mapq, n_want, want_k, the record array and both pools byte for byte.  Slices of tests/phase2gen.py at the kernels' block sizes,
regions the sort moves before bwa_fix_xref2 or the host's redo gets them, every refusal with the outputs and the vectors untouched,
the session's uploads and waits in numbers, and the switch behind bmh_sam_batch."""
import ctypes as C

import numpy as np
import pytest

import decidegen as dg
import kswgen
import kswlib
import phase2gen as pg
import wantgen as wg
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_CIGAR_CAP = -3, -4, -6
MOVED, HOST = 4, 8


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ref():
    return wg.reference()


@pytest.fixture(scope="module")
def ctx(pkg, ref):
    c = pkg.Context(0, kswlib.make_params())
    c.idx = pkg.make_refidx(wg.CONTIGS)
    c.pac = c.set_pac(ref[1], wg.L_PAC)
    c.set_refidx(c.idx)
    yield c
    c.close()


def _host(pkg, c, o, pes, id0, reads, vectors):
    """the yardstick: bmh_decide_batch, then bmh_wanted_cigar_batch over what it left"""
    a = pkg.decide_batch(o, c.idx.l_pac, pes, id0, vectors)
    res, cig, md = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), reads, a["regs"], [list(k) for k in a["want"]])
    return a, res, cig, md


def _same(dev, host, what):
    a, hr, hc, hm = host
    dg.assert_same(dev, a, what)
    assert dev["n_wanted"] == len(hr) == len(dev["res"]), (what, dev["n_wanted"], len(hr))
    bad = [j for j in range(len(hr)) if dev["res"][j].tobytes() != hr[j].tobytes()]
    assert not bad, (what, len(bad), bad[:5], dev["res"][bad[0]], hr[bad[0]])
    cu, mu = int(hr["n_cigar"].sum()), int((hr["md_len"].astype(np.int64) + 1).sum())
    assert np.array_equal(dev["cig"][:cu], hc[:cu]) and bytes(dev["md"][:mu]) == bytes(hm[:mu]), what


def _both(pkg, c, o, pes, id0, reads, vectors, what):
    host = _host(pkg, c, o, pes, id0, reads, vectors)
    dev = c.phase2_device(o, c.idx, c.pac, pes, id0, reads, vectors)
    _same(dev, host, what)
    st = c.last_phase2_stats()
    units = len(reads) // 2 if int(o["flag"]) & pg.PE else len(reads)
    assert (st["units"], st["wanted"], st["fallbacks"], st["sessions"]) == (units, len(host[1]), 0, 1), (what, st)
    assert st["waits"] <= 3, (what, st)
    assert c.last_decide_stats()[:2] == (units, 0) and c.last_wanted_stats()[:3] == (st["wanted"], st["fixed"], st["redone"]), what
    return host, st


def _with_w(c, w):
    c.set_params(kswlib.make_params(w=w))


@pytest.mark.parametrize("w", [100, 5])
@pytest.mark.parametrize("mode", ["se", "pe"])
@pytest.mark.parametrize("units", [1, 63, 64, 65, 130])
def test_unit_counts(pkg, ctx, units, mode, w):
    """decide_kernel's 64-lane blocks: one unit, around a block, two blocks and a little"""
    o, pes, id0, reads, vectors = pg.make(mode, units=units, w=w)
    assert len(reads) == (2 * units if mode == "pe" else units)
    _with_w(ctx, w)
    try:
        _both(pkg, ctx, o, pes, id0, reads, vectors, f"{units} units, {mode}, w={w}")
    finally:
        _with_w(ctx, 100)


@pytest.mark.parametrize("w", [100, 5])
@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
@pytest.mark.parametrize("n_wanted", [1, 255, 256, 257, 1023, 1024, 1025, 1500])
def test_wanted_counts(pkg, ctx, n_wanted, mode, w):
    """the planning kernels' 256-lane blocks and the scan's 1024-lane tiles: one region, around a block, around a tile, two tiles"""
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=n_wanted, w=w)
    _with_w(ctx, w)
    try:
        (a, res, _, _), st = _both(pkg, ctx, o, pes, id0, reads, vectors, f"{n_wanted} wanted, {mode}, w={w}")
    finally:
        _with_w(ctx, 100)
    assert len(res) == n_wanted and st["redone"] == 0 and not (res["flags"] != 0).any()
    if n_wanted < 1023:
        return
    s = pg.shapes(o, vectors, a)
    assert s["no_region"] >= 16 and s["none_wanted"] >= 16, s
    assert s["moved_first"] >= 32, s  # a session that plans from the unsorted regions fails on these
    if mode.endswith("all"):
        assert s["multi_secondary"] >= 32, s
    if mode == "se":
        assert s["total"] >= 2 * s["n_w"], s  # the capacity is more than twice the count
    if mode.startswith("pe"):
        pairs = len(reads) // 2
        assert 3 * s["paired"] >= pairs and 10 * s["unpaired"] >= pairs, s


def test_no_region_and_no_read(pkg, ctx, ref):
    """reads without regions still get pass A's verdicts; n == 0 runs nothing"""
    rng = np.random.default_rng(5)
    reads = [kswgen.rand_seq(rng, 50) for _ in range(6)]
    vectors = [np.zeros(0, dtype=kswlib.ALNREG) for _ in reads]
    for mode in ("se", "pe"):
        o, pes = pg.opt(100, pg.PE if mode == "pe" else 0), (pg.pes_fr() if mode == "pe" else None)
        dev = ctx.phase2_device(o, ctx.idx, ctx.pac, pes, 10, reads, vectors)
        dg.assert_same(dev, pkg.decide_batch(o, wg.L_PAC, pes, 10, vectors), mode)
        assert dev["n_wanted"] == 0 and ctx.last_phase2_stats()["sessions"] == 1
    dev = ctx.phase2_device(pg.opt(), ctx.idx, ctx.pac, None, 10, [], [])
    st = ctx.last_phase2_stats()
    assert dev["n_wanted"] == 0 and (st["units"], st["wanted"], st["sessions"], st["waits"], st["h2d_bytes"]) == (0, 0, 0, 0, 0)


def _behind(rng, whole, rd, reg):
    """(read, vector) with the constructed region first and an ordinary region of the same read, 25 points better, second: the sort
    moves the constructed one back"""
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
    o = pg.opt()
    fr, fv = pg.se_slice(rng, whole, 40)
    reads, vectors = list(fr[:20]), list(fv[:20])
    for name, rd, reg, expect in cases:
        b, v = _behind(rng, whole, rd, reg)
        reads.append(b), vectors.append(v)
    reads += fr[20:]
    vectors += fv[20:]
    (a, res, _, _), st = _both(pkg, ctx, o, None, 300, reads, vectors, "overhangs")
    n_fix = sum(c[3] != "none" for c in cases)
    for i, (name, rd, reg, expect) in enumerate(cases):  # moved to index 1, and wanted there
        v = a["regs"][20 + i]
        assert (int(v[1]["qb"]), int(v[1]["qe"])) == (0, len(rd)) and list(a["want"][20 + i]) == [0, 1], name
    assert n_fix >= 32 and st["fixed"] == n_fix and st["redone"] == 0, (n_fix, st)
    assert int(((res["flags"] & MOVED) != 0).sum()) == n_fix


def _long_reference(pkg, seed, l_pac):
    whole = kswgen.rand_seq(np.random.default_rng(seed), l_pac)
    c = pkg.Context(0, kswlib.make_params())
    c.idx = pkg.make_refidx([(0, l_pac // 2), (l_pac // 2, l_pac - l_pac // 2)])
    c.pac = c.set_pac(wg.pack(whole), l_pac)
    c.set_refidx(c.idx)
    return whole, c


def test_alignments_that_outgrow_the_slots_are_redone_from_the_sorted_block(pkg):
    """a substitution every 3 bases of 250: an MD past the 128 bytes of its slot; 14 separated indels: a CIGAR past 24 words.  Each is
    the second region of its input vector and the first after the sort, so a redo that took its record from the caller's vectors
    would align the wrong region; the rest of the slice is not redone."""
    whole, c = _long_reference(pkg, 60, 20000)
    try:
        rng = np.random.default_rng(61)
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
            rb, re = (pos, pos + tl) if not rev else (40000 - pos - tl, 40000 - pos)
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
        (a, res, _, _), st = _both(pkg, c, pg.opt(), None, 50, reads, vectors, "long MD and CIGAR")
        assert len(special) == 8 and st["redone"] == 8 and st["wanted"] == 24 + 8 and st["fixed"] == 0
        j = 0
        for k in range(24):
            if k in special:
                assert int(a["regs"][k][0]["qb"]) == 120 and list(a["want"][k]) == [0, 1]  # the sort brought it to the front
                assert int(res["flags"][j]) == HOST and int(res["flags"][j + 1]) == 0, (k, res[j], res[j + 1])
                assert int(res["md_len"][j]) > 128 if k % 6 == 2 else int(res["n_cigar"][j]) > 24
            else:
                assert int(res["flags"][j]) == 0, (k, res[j])
            j += len(a["want"][k])
    finally:
        c.close()


@pytest.mark.parametrize("n_w", [2, 1])
def test_no_record_in_the_main_round(pkg, n_w):
    """wantgen.long_fixes' regions alone, each the one region of its read: every wanted region is the host's after round 0, so the main
    round has no record, no slot comes down and every record is redone from the sorted block"""
    whole, c = _long_reference(pkg, 70, 20000)
    try:
        b = 10000
        reads, vectors = [], []
        for rd, reg in wg.long_fixes(whole, b, score=300)[:n_w]:
            reg["seedcov"] = 60
            reads.append(rd), vectors.append(np.array([reg], dtype=kswlib.ALNREG))
        (a, res, _, _), st = _both(pkg, c, pg.opt(), None, 50, reads, vectors, f"{n_w} long fixes alone")
        assert [list(k) for k in a["want"]] == [[0]] * n_w
        assert list(res["flags"]) == [MOVED | HOST] * n_w and int(res["re"][0]) == b
        assert n_w < 2 or int(res["rb"][1]) == 40000 - b
        assert (st["wanted"], st["fixed"], st["redone"]) == (n_w, n_w, n_w) and c.last_wanted_stats()[:3] == (n_w, n_w, n_w)
    finally:
        c.close()


# ---------------------------------------------------------------- refusals: all or nothing

def _sentinels(pkg, o, vectors):
    total, n = sum(len(v) for v in vectors), len(vectors)
    return {"pd": np.frombuffer(b"\x5a" * (48 * (n // 2 if int(o["flag"]) & pg.PE else 0)), dtype=pkg.PAIRDEC).copy(),
            "reg_mapq": np.full(total, 0x5a5a5a5a, dtype=np.int32), "want_k": np.full(total, 0x5a5a5a5a, dtype=np.int32),
            "n_want": np.full(n, 0x5a5a5a5a, dtype=np.int32), "res": np.frombuffer(b"\x5a" * (72 * total), dtype=pkg.WANTED_RES).copy(),
            "cig": np.full(400 * total + 64, 0xa5a5a5a5, dtype=np.uint32), "md": np.full(1200 * total + 64, 0x5a, dtype=np.uint8)}


def _refused(pkg, c, o, pes, reads, vectors, code, idx=None, pac=None, out=None, results_cap=None):
    """the call fails with `code`; every output keeps its sentinel bytes and the vectors are the input's, not even sorted"""
    vectors = [np.ascontiguousarray(v, dtype=kswlib.ALNREG).copy() for v in vectors]
    before = [v.tobytes() for v in vectors]
    out = {**_sentinels(pkg, o, vectors), **(out or {})}
    keep = {k: v.copy() for k, v in out.items()}
    with pytest.raises(pkg.BmhError) as e:
        c.phase2_device(o, idx if idx is not None else c.idx, pac if pac is not None else c.pac, pes, 40, reads, vectors, inplace=True, out=out,
                        results_cap=results_cap)
    assert e.value.code == code, e.value
    for k in out:
        assert out[k].tobytes() == keep[k].tobytes(), k
    assert [v.tobytes() for v in vectors] == before


def _ordinary(pkg, c, seed=41):
    """the context is as good as before"""
    o, pes, id0, reads, vectors = pg.make("se", units=50, seed=seed)
    _both(pkg, c, o, pes, id0, reads, vectors, "after a refused call")


@pytest.mark.parametrize("which", ["lost", "bridge"])
def test_a_region_the_reference_aborts_on_fails_the_whole_call(pkg, ctx, ref, which):
    whole = ref[0]
    rd, reg = wg.lost_region(whole) if which == "lost" else wg.bridging_region(whole)
    assert int(reg["score"]) >= pg.T  # pass A wants it
    o, pes, id0, reads, vectors = pg.make("se", units=30, seed=12)
    reads.insert(11, rd), vectors.insert(11, np.array([reg], dtype=kswlib.ALNREG))
    assert list(pkg.decide_batch(o, wg.L_PAC, None, 40, vectors)["want"][11]) == [0]
    _refused(pkg, ctx, o, pes, reads, vectors, E_ARG)
    _ordinary(pkg, ctx)


def test_a_wanted_window_past_65535_is_out_of_range(pkg):
    whole, c = _long_reference(pkg, 42, 80000)
    try:
        rd = whole[100:250].copy()
        a = wg.region(0, 150, 100, 100 + 65536, 150, 100, 150)
        b = wg.region(0, 150, 100, 250, 150, 100, 150)
        for x in (a, b):
            x["seedcov"] = 100
        o = pg.opt()
        _refused(pkg, c, o, None, [rd], [np.array([a], dtype=kswlib.ALNREG)], E_RANGE)
        assert c.last_phase2_stats()["fallbacks"] == 0  # a kernel's refusal, not the tables'
        dev = c.phase2_device(o, c.idx, c.pac, None, 40, [rd], [np.array([b], dtype=kswlib.ALNREG)])
        _same(dev, _host(pkg, c, o, None, 40, [rd], [np.array([b], dtype=kswlib.ALNREG)]), "the same read with a window that fits")
        # unwanted, the long window is no obstacle
        a["score"] = pg.T - 1
        assert c.phase2_device(o, c.idx, c.pac, None, 40, [rd], [np.array([a], dtype=kswlib.ALNREG)])["n_wanted"] == 0
    finally:
        c.close()


def test_capacities_too_small(pkg, ctx):
    o, pes, id0, reads, vectors = pg.make("se-all", n_wanted=70, seed=3)
    _, res, _, _ = _host(pkg, ctx, o, pes, 40, reads, vectors)
    cu, mu = int(res["n_cigar"].sum()), int((res["md_len"].astype(np.int64) + 1).sum())
    _refused(pkg, ctx, o, pes, reads, vectors, E_CIGAR_CAP, results_cap=len(res) - 1)
    _refused(pkg, ctx, o, pes, reads, vectors, E_CIGAR_CAP, out={"cig": np.full(cu - 1, 0xa5a5a5a5, dtype=np.uint32)})
    _refused(pkg, ctx, o, pes, reads, vectors, E_CIGAR_CAP, out={"md": np.full(mu - 1, 0x5a, dtype=np.uint8)})
    # exactly enough of each
    total = sum(len(v) for v in vectors)
    out = {"res": np.zeros(total, dtype=pkg.WANTED_RES), "cig": np.zeros(cu, dtype=np.uint32), "md": np.zeros(mu, dtype=np.uint8)}
    dev = ctx.phase2_device(o, ctx.idx, ctx.pac, pes, 40, reads, vectors, out=out, results_cap=len(res))
    _same(dev, _host(pkg, ctx, o, pes, 40, reads, vectors), "exact capacities")


def test_refusals_without_the_resident_tables(pkg, ref):
    o, pes, id0, reads, vectors = pg.make("se", units=10, seed=43)
    c = pkg.Context(0, kswlib.make_params())
    try:
        c.idx, c.pac = pkg.make_refidx(wg.CONTIGS), ref[1]
        _refused(pkg, c, o, pes, reads, vectors, E_ARG)  # neither
        c.set_refidx(c.idx)
        _refused(pkg, c, o, pes, reads, vectors, E_ARG)  # no reference
        c.pac = c.set_pac(ref[1], wg.L_PAC)
        _both(pkg, c, o, pes, id0, reads, vectors, "both resident")
        c.set_refidx(None)
        _refused(pkg, c, o, pes, reads, vectors, E_ARG)  # the table dropped
        c.set_refidx(c.idx)
        _ordinary(pkg, c)
    finally:
        c.close()
    raw = pkg.Context(0)  # no parameters either
    try:
        raw.idx = pkg.make_refidx(wg.CONTIGS)
        raw.pac = raw.set_pac(ref[1], wg.L_PAC)
        raw.set_refidx(raw.idx)
        _refused(pkg, raw, o, pes, reads, vectors, E_ARG)
    finally:
        raw.close()


def test_tables_past_their_limit_are_refused_before_any_upload(pkg, ctx):
    o, pes, id0, reads, vectors = pg.make("pe", units=40, seed=9)
    _both(pkg, ctx, o, pes, id0, reads, vectors, "the model that fits")
    _refused(pkg, ctx, o, dg.special_pes("wide"), reads, vectors, E_RANGE)
    st = ctx.last_phase2_stats()
    assert (st["fallbacks"], st["sessions"], st["h2d_bytes"], st["waits"]) == (1, 0, 0, 0), st
    with pytest.raises(pkg.BmhError) as e:  # odd n with PE: what bmh_decide_batch refuses
        ctx.phase2_device(o, ctx.idx, ctx.pac, pes, 40, reads[:-1], vectors[:-1])
    assert e.value.code == E_ARG
    _ordinary(pkg, ctx)


# ---------------------------------------------------------------- one session, in numbers

def test_one_upload_and_three_waits(pkg, ref):
    o, pes, id0, reads, vectors = pg.make("pe", n_wanted=1500)
    total, n = sum(len(v) for v in vectors), len(reads)
    reads_bytes = sum(len(r) for r in reads)
    assert total * 64 > 64 << 10
    bound = total * 64 + reads_bytes + 16 * (n + 1) + 8 * pg.N_TERM + (8 << 10)
    c = pkg.Context(0, kswlib.make_params())
    try:
        c.idx = pkg.make_refidx(wg.CONTIGS)
        c.pac = c.set_pac(ref[1], wg.L_PAC)
        c.set_refidx(c.idx)
        _, first = _both(pkg, c, o, pes, id0, reads, vectors, "the call that makes the log table")
        _, again = _both(pkg, c, o, pes, id0, reads, vectors, "the next call")
        for st, log_bytes in ((first, 8 << 17), (again, 0)):
            assert st["waits"] <= 3 and st["sessions"] == 1, st
            # the regions once: a second upload of them, or of the want list, breaks the bound
            assert total * 64 < st["h2d_bytes"] <= bound + log_bytes, (st, bound)
        assert first["h2d_bytes"] - again["h2d_bytes"] == 8 << 17
        # down: pass A's block, the records, the slots of the regions aligned -- not a capacity's worth of slots
        n_w = again["wanted"]
        assert again["d2h_bytes"] <= total * 72 + 4 * n + 24 * n + n_w * (72 + 96 + 128) + (8 << 10), again
        c.set_kernel_timing(True)
        _, timed = _both(pkg, c, o, pes, id0, reads, vectors, "timed")
        assert timed["decide_ms"] > 0 and timed["wanted_ms"] > 0 and again["decide_ms"] == -1 and again["wanted_ms"] == -1
    finally:
        c.close()


# ---------------------------------------------------------------- the switch behind bmh_sam_batch

class _Seq(C.Structure):  # bmh_seq_t
    _fields_ = [("l_seq", C.c_int32), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


def _sam_batch(pkg, c, o, pes, id0, vecs, reads):
    lib = pkg.lib()
    lib.bmh_sam_batch.restype = C.c_int
    seqs = (_Seq * max(len(reads), 1))()
    keep = []
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        keep.append(r)
        seqs[i] = _Seq(len(r), b"r%d" % (i // 2 if int(o["flag"]) & pg.PE else i), None, r.ctypes.data, None, None)
    bufs = [np.array(v, dtype=kswlib.ALNREG, copy=True) for v in vecs]
    c_regs = (kswlib.CAlnregV * max(len(bufs), 1))()
    for i, a in enumerate(bufs):
        c_regs[i].n = c_regs[i].m = len(a)
        c_regs[i].a = a.ctypes.data if len(a) else None
    rc = lib.bmh_sam_batch(c._h, o.ctypes.data_as(C.c_void_p), C.byref(c.idx), c.pac.ctypes.data_as(C.c_void_p),
                           pes.ctypes.data_as(C.c_void_p) if pes is not None else None, C.c_int64(id0), len(reads), seqs, c_regs, b"")
    assert rc == 0, (rc, lib.bmh_last_error(c._h))
    text = []
    for s in seqs[:len(reads)]:
        text.append(C.string_at(s.sam))
        pkg._libc.free(C.c_void_p(s.sam))
    return text, [a.tobytes() for a in bufs]


_COUNTED = ("units", "wanted", "fixed", "redone", "fallbacks", "h2d_bytes", "d2h_bytes", "waits", "sessions")


@pytest.mark.parametrize("mode", ["se", "pe"])
def test_switch_behind_sam_batch(pkg, ref, mode):
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=400, seed=31)
    rng = np.random.default_rng(32)
    for name, rd, reg, expect in wg.overhangs(ref[0])[:6]:  # some regions to fix, behind the sort
        b, v = _behind(rng, ref[0], rd, reg)
        reads += [b, kswgen.rand_seq(rng, 60)] if mode == "pe" else [b]
        vectors += [v, np.zeros(0, dtype=kswlib.ALNREG)] if mode == "pe" else [v]
    c = pkg.Context(0, kswlib.make_params())
    try:
        c.idx = pkg.make_refidx(wg.CONTIGS)
        c.pac = c.set_pac(ref[1], wg.L_PAC)
        c.set_refidx(c.idx)
        t0, r0 = _sam_batch(pkg, c, o, pes, id0, vectors, reads)
        assert c.last_phase2_stats()["sessions"] == -1  # nothing fused yet
        _both(pkg, c, o, pes, id0, reads, vectors, "direct, the log table made")
        _, direct = _both(pkg, c, o, pes, id0, reads, vectors, "direct")
        c.set_phase2_device(True)
        t1, r1 = _sam_batch(pkg, c, o, pes, id0, vectors, reads)
        assert t0 == t1 and r0 == r1
        st = c.last_phase2_stats()
        assert {k: st[k] for k in _COUNTED} == {k: direct[k] for k in _COUNTED}
        mapped = sum(1 for t in t0 for l in t.splitlines() if not int(l.split(b"\t")[1]) & 4)
        assert st["wanted"] == mapped and st["fixed"] >= 4 and st["sessions"] == 1 and st["waits"] <= 3, (st, mapped)
        # the other two switches do not matter while this one is on
        c.set_decide_device(True), c.set_wanted_device(True)
        t2, r2 = _sam_batch(pkg, c, o, pes, id0, vectors, reads)
        assert t0 == t2 and r0 == r2 and c.last_phase2_stats()["sessions"] == 1
        # a call that returns before its passes leaves its own statistics, not the previous slice's
        assert _sam_batch(pkg, c, o, pes, id0, [], []) == ([], [])
        st = c.last_phase2_stats()
        assert (st["units"], st["wanted"], st["sessions"], st["h2d_bytes"], st["waits"]) == (0, 0, 0, 0, 0), st
        if mode == "pe":  # a window the pair table cannot hold: the slice goes the way the other two switches say
            wide = dg.special_pes("wide")
            for two in (False, True):
                c.set_phase2_device(False), c.set_decide_device(False), c.set_wanted_device(False)
                t3, r3 = _sam_batch(pkg, c, o, wide, id0, vectors, reads)
                c.set_phase2_device(True), c.set_decide_device(two), c.set_wanted_device(two)
                t4, r4 = _sam_batch(pkg, c, o, wide, id0, vectors, reads)
                assert t3 == t4 and r3 == r4
                st = c.last_phase2_stats()
                assert (st["fallbacks"], st["sessions"]) == (1, 2), st
                if two:
                    assert c.last_decide_stats()[:2] == (0, 1) and c.last_wanted_stats()[0] > 0
        # off again: nothing fused, the statistics stay
        c.set_phase2_device(False), c.set_decide_device(False), c.set_wanted_device(False)
        before = c.last_phase2_stats()
        t5, r5 = _sam_batch(pkg, c, o, pes, id0, vectors, reads)
        assert t0 == t5 and r0 == r5 and c.last_phase2_stats() == before
    finally:
        c.close()
