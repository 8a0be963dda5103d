"""bmh_decide_device (csrc/decide.hip: decide_kernel, one lane per read or pair, over host/postproc_core.h) against bmh_decide_batch,
the gcc build of the same text: regions byte for byte, the pair verdicts, reg_mapq, n_want, want_k -- and on the single-end fixture
against the compiled reference's records directly.  Then the switch behind bmh_sam_batch: same text, same vectors."""
import ctypes as C

import numpy as np
import pytest

import decidegen as dg
import kswgen
import kswlib
import postgen
import sortmodel as sm
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -3, -4


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
    units, fallbacks, _ = ctx.last_decide_stats()
    assert (units, fallbacks) == (len(vecs) // 2 if int(o["flag"]) & dg.PE else len(vecs), 0), what
    return dev


@pytest.mark.parametrize("si", range(len(postgen.OPTION_SETS)))
def test_single_end_fixture(pkg, ctx, si):
    o, vecs, marked, mapq = dg.se_fixture(si)
    dev = _both(pkg, ctx, o, dg.L_PAC, None, dg.SE_ID0, dg.se_spread(vecs), f"set {si}")
    assert np.concatenate(dev["regs"]).tobytes() == np.ascontiguousarray(marked, dtype=kswlib.ALNREG).tobytes()
    assert (dev["reg_mapq"] == mapq).all()


@pytest.mark.parametrize("units", [1, 63, 64, 65, 1400])
def test_unit_counts(pkg, ctx, units):
    """the last block is partly empty: single-end reads, then as many pairs"""
    o, vecs, _, _ = dg.se_fixture(0)
    reads = [vecs[i % len(vecs)] for i in range(units)]  # (the fixture has 350 vectors: repeated, each with another id)
    assert len(reads) == units
    _both(pkg, ctx, o, dg.L_PAC, None, 99, reads, f"{units} reads")
    _both(pkg, ctx, dg.pe_opt(0), dg.L_PAC, dg.fixture_pes(0), 2000, dg.pe_vectors(1000 + units, units), f"{units} pairs")


def test_vector_sizes_at_the_sorts_borders(pkg, ctx):
    """0, 1, 2, 16, 17, 33 and 40 regions: no sort, the two-record exchange, insertion sort only, quicksort with and without a
    pushed range -- as reads and as the two ends of pairs (whose key array then has up to 80 records)"""
    sizes = [0, 1, 2, 16, 17, 33, 40]
    vecs = dg.vectors_of_sizes(np.random.default_rng(3), sizes + sizes[::-1] + [40, 40, 0, 40, 17, 16])
    _both(pkg, ctx, dg.sam_opt(), 3_000_000, None, 5, vecs, "reads")
    for si in (0, 2):
        dev = _both(pkg, ctx, dg.pe_opt(si), 3_000_000, dg.fixture_pes(si), 6, vecs, f"pairs, set {si}")
        assert len(dev["pd"]) == len(vecs) // 2


def test_combsort_cases_of_the_sort_fixture(pkg, ctx):
    """the marking's sort in its combsort fallback (tests/test_sort_paths_cpu.py proves the path): the reference's columns and CRC"""
    fx = sm.fixture()
    o = dg.sam_opt()
    picked = [ci for ci, a in enumerate(fx["reg_want"][0.95]) if len(a) <= 300]
    longest = 0
    for ci in picked:  # ids 12345 + 7 ci: one call each
        (name, _), a = fx["regs"][ci], fx["reg_want"][0.95][ci]
        dev = _both(pkg, ctx, o, 3_000_000, None, 12345 + 7 * ci, [a], name)
        got = dev["regs"][0]
        cols = np.stack([got[k].astype(np.int64) for k in sm.MARK_FIELDS], axis=1) if len(got) else np.zeros((0, len(sm.MARK_FIELDS)), np.int64)
        assert (cols == fx["reg_marked"][ci]).all(), name
        assert sm.crc(got) == fx["reg_marked_crc"][ci], name
        if len(a) >= 280:
            c = sm.trace_mark_sort(a, got).comb
            longest = max(longest, max(c) if c else 0)
    assert len(picked) > 20 and longest >= 280, (len(picked), longest)


@pytest.mark.parametrize("case", ["empty_end", "none", "std0", "nopairing", "all", "nopairing_all", "set2_seedcov0"])
def test_special_pairs(pkg, ctx, case):
    vecs = dg.pe_vectors(21, 150)
    o, pes = dg.pe_opt(0), dg.fixture_pes(0)
    if case == "empty_end":
        for p in range(0, 150, 3):
            vecs[2 * p + p % 2] = vecs[2 * p + p % 2][:0]
    elif case in ("none", "std0"):
        pes = dg.special_pes(case)
    elif case == "set2_seedcov0":  # mapQ_coef_len = 0: log(seedcov), and log(0.) for a seedcov of 0
        o, pes = dg.pe_opt(2), dg.fixture_pes(2)
        for v in vecs[::3]:
            if len(v):
                v[0]["seedcov"] = 0
    else:
        o = dg.pe_opt(0, {"nopairing": dg.NOPAIRING, "all": dg.ALL, "nopairing_all": dg.NOPAIRING | dg.ALL}[case])
    dev = _both(pkg, ctx, o, dg.L_PAC, pes, 10, vecs, case)
    paired = int(dev["pd"]["paired"].sum())
    if case in ("none", "nopairing", "nopairing_all"):
        assert paired == 0 and (dev["pd"]["score"] == 0).all()
    elif case == "std0":
        assert (dev["pd"]["score"] >= 0).all()  # erfc -> 0 or NaN: q = INT32_MIN, clamped to 0 like the reference's
    else:
        assert paired > 30
    if case == "set2_seedcov0":
        _both(pkg, ctx, dg.sam_opt(**postgen.OPTION_SETS[2]), dg.L_PAC, None, 10, vecs, case + " single-end")


@pytest.mark.parametrize("id0", dg.ID0_TRUNCATING)
def test_ids_where_mem_pair_truncates(pkg, ctx, id0):
    dev = _both(pkg, ctx, dg.pe_opt(0), dg.L_PAC, dg.fixture_pes(0), id0, dg.pe_vectors(9, 60), f"id0 {id0}")
    assert dev["pd"]["paired"].sum() > 10


def test_refusals_leave_the_vectors_untouched(pkg, ctx):
    o = dg.pe_opt(0)
    vecs = [np.ascontiguousarray(v) for v in dg.pe_vectors(9, 40)]
    before = [v.tobytes() for v in vecs]
    with pytest.raises(pkg.BmhError) as e:
        ctx.decide_device(o, dg.L_PAC, dg.special_pes("wide"), 0, vecs, inplace=True)
    assert e.value.code == E_RANGE
    assert [v.tobytes() for v in vecs] == before
    assert ctx.last_decide_stats()[:2] == (0, 1)
    roff = np.cumsum([0] + [len(v) for v in vecs])
    roff[3] -= 1
    with pytest.raises(pkg.BmhError) as e:
        ctx.decide_device(o, dg.L_PAC, dg.fixture_pes(0), 0, vecs, roff=roff, inplace=True)
    assert e.value.code == E_ARG
    assert [v.tobytes() for v in vecs] == before
    # the same window is no obstacle where nothing pairs, and n == 0 is no launch
    out = ctx.decide_device(dg.pe_opt(0, dg.NOPAIRING), dg.L_PAC, dg.special_pes("wide"), 0, vecs)
    dg.assert_same(out, pkg.decide_batch(dg.pe_opt(0, dg.NOPAIRING), dg.L_PAC, dg.special_pes("wide"), 0, vecs))
    assert len(ctx.decide_device(o, dg.L_PAC, dg.fixture_pes(0), 0, [])["pd"]) == 0 and ctx.last_decide_stats()[:2] == (0, 0)
    # a region longer than the log table may reach
    long_v = np.zeros(1, dtype=kswlib.ALNREG)
    long_v[0]["re"], long_v[0]["qe"], long_v[0]["score"] = 1 << 21, 100, 100
    with pytest.raises(pkg.BmhError) as e:
        ctx.decide_device(dg.sam_opt(), 3_000_000, None, 0, [long_v])
    assert e.value.code == E_RANGE


# ---------------------------------------------------------------- the switch behind bmh_sam_batch

class _Ann(C.Structure):  # bmh_refann_t
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("name", C.c_char_p), ("anno", C.c_char_p)]


class _Idx(C.Structure):  # bmh_refidx_t
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(_Ann))]


class _Seq(C.Structure):  # bmh_seq_t
    _fields_ = [("l_seq", C.c_int32), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


def _sam_batch(pkg, ctx, o, pes, id0, vecs, ref, reads):
    """bmh_sam_batch over a one-sequence reference -> (the SAM text per read, the vectors as it leaves them)"""
    lib = pkg.lib()
    lib.bmh_sam_batch.restype = C.c_int
    l_pac = len(ref)
    pac = np.zeros((l_pac + 3) // 4, dtype=np.uint8)
    for k in range(4):
        part = ref[k::4].astype(np.uint8)
        pac[:len(part)] |= part << ((3 - k) * 2)
    ann = (_Ann * 1)(_Ann(0, l_pac, 0, 0, b"synth", b""))
    idx = _Idx(l_pac, 1, 11, ann)
    seqs = (_Seq * len(reads))()
    keep = []
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        keep.append(r)
        seqs[i] = _Seq(len(r), b"r%d" % (i // 2 if int(o["flag"]) & dg.PE else i), None, r.ctypes.data, None, None)
    bufs = [np.array(v, dtype=kswlib.ALNREG, copy=True) for v in vecs]
    c_regs = (kswlib.CAlnregV * len(bufs))()
    for i, a in enumerate(bufs):
        c_regs[i].n = c_regs[i].m = len(a)
        c_regs[i].a = a.ctypes.data if len(a) else None
    rc = lib.bmh_sam_batch(ctx._h, o.ctypes.data_as(C.c_void_p), C.byref(idx), pac.ctypes.data_as(C.c_void_p),
                           pes.ctypes.data_as(C.c_void_p) if pes is not None else None, C.c_int64(id0), len(reads), seqs, c_regs, b"")
    assert rc == 0, (rc, lib.bmh_last_error(ctx._h))
    text = []
    for s in seqs:
        text.append(C.string_at(s.sam))
        pkg._libc.free(C.c_void_p(s.sam))
    return text, [a.tobytes() for a in bufs]


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_switch_behind_sam_batch(pkg, ctx, paired):
    rng = np.random.default_rng(31)
    ref = kswgen.rand_seq(rng, dg.L_PAC)
    if paired:
        vecs = dg.pe_vectors(33, 300)
        o, pes = dg.pe_opt(0), dg.fixture_pes(0)
    else:
        vecs = postgen.region_vectors(rng, 400, dg.L_PAC)
        o, pes = dg.sam_opt(), None
    # a region must lie on one strand, inside the reference
    ok = [all(0 <= int(r["rb"]) and int(r["re"]) <= 2 * dg.L_PAC and not int(r["rb"]) < dg.L_PAC < int(r["re"]) for r in v) for v in vecs]
    if paired:
        ok = [a and b for a, b in zip(ok[::2], ok[1::2]) for _ in range(2)]
    vecs = [v for v, k in zip(vecs, ok) if k]
    assert len(vecs) > 300
    reads = [kswgen.rand_seq(rng, 150) for _ in vecs]
    try:
        ctx.set_decide_device(False)
        t0, r0 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, ref, reads)
        ctx.set_decide_device(True)
        t1, r1 = _sam_batch(pkg, ctx, o, pes, 4000, vecs, ref, reads)
        assert t0 == t1 and r0 == r1
        assert ctx.last_decide_stats()[:2] == (len(vecs) // 2 if paired else len(vecs), 0)
        assert sum(len(t.splitlines()) for t in t0) >= len(vecs)
        # a call that returns before its decisions leaves its own statistics, not the previous slice's
        assert _sam_batch(pkg, ctx, o, pes, 4000, [], ref, []) == ([], []) and ctx.last_decide_stats()[:2] == (0, 0)
        if paired:  # a window the pair table cannot hold: the slice is decided on the host, same text
            wide = dg.special_pes("wide")
            ctx.set_decide_device(False)
            t2, r2 = _sam_batch(pkg, ctx, o, wide, 4000, vecs, ref, reads)
            ctx.set_decide_device(True)
            t3, r3 = _sam_batch(pkg, ctx, o, wide, 4000, vecs, ref, reads)
            assert t2 == t3 and r2 == r3
            assert ctx.last_decide_stats()[:2] == (0, 1)
    finally:
        ctx.set_decide_device(False)
