"""bmh_sam_text_device -- samtext_size_kernel, the scan, samtext_emit_kernel -- against bmh_sam_text_batch: the text and text_off byte
for byte.  The constructed slices of tests/samtextgen.py at unit counts around the kernels' blocks, phase2gen's slices through the host's
pass A and pass B, every refusal with the outputs untouched, the session's uploads and waits in numbers, a text buffer that grows, and
the switch behind bmh_sam_batch."""
import ctypes as C

import numpy as np
import pytest

import kswlib
import phase2gen as pg
import samtextgen as sg
import wantgen as wg
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # (needs neither parameters nor the 2-bit reference)
    c.idx = sg.refidx()
    c.set_refidx(c.idx), c.set_refnames(c.idx)
    yield c
    c.close()


def _args(sl, idx):
    return (sl["opt"], idx, sl["pes"], sl["seqs"], sl["vectors"], sl["dec"], sl["res"], sl["cig"], sl["md"], sl["rg_id"])


def _both(pkg, c, sl, what, idx=None):
    a = _args(sl, idx if idx is not None else c.idx)
    ht, hoff = pkg.sam_text_batch(*a)
    dt, doff = c.sam_text_batch(*a)
    assert np.array_equal(hoff, doff), (what, np.flatnonzero(hoff != doff)[:5])
    if dt != ht:
        i = next(i for i in range(len(hoff) - 1) if dt[int(hoff[i]):int(hoff[i + 1])] != ht[int(hoff[i]):int(hoff[i + 1])])
        raise AssertionError((what, i, dt[int(hoff[i]):int(hoff[i + 1])][:400], ht[int(hoff[i]):int(hoff[i + 1])][:400]))
    st = c.last_samtext_stats()
    assert (st["reads"], st["lines"], st["text_bytes"], st["waits"]) == (len(sl["seqs"]), ht.count(b"\n"), len(ht), 2), (what, st)
    return ht, st


@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
@pytest.mark.parametrize("units", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_unit_counts(pkg, ctx, units, mode):
    _both(pkg, ctx, sg.make(mode, units, seed=units), f"{mode} {units}")


@pytest.mark.parametrize("mode,flag", [("se", sg.NO_MULTI), ("pe-all", sg.NO_MULTI), ("pe", sg.NOPAIRING)])
def test_other_flags(pkg, ctx, mode, flag):
    _both(pkg, ctx, sg.make(mode, 130, seed=5, flag=flag), f"{mode} flag {flag:#x}")


@pytest.fixture(scope="module")
def real(pkg):
    """a context over wantgen's reference, for pass B and bmh_sam_batch"""
    whole, pac = wg.reference()
    c = pkg.Context(0, kswlib.make_params())
    c.idx = pkg.make_refidx(wg.CONTIGS)
    c.pac = c.set_pac(pac, wg.L_PAC)
    c.set_refidx(c.idx), c.set_refnames(c.idx)
    yield c
    c.close()


def _phase2_slice(pkg, c, mode, n_wanted, seed=0):
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=n_wanted, seed=seed)
    a = pkg.decide_batch(o, c.idx.l_pac, pes, id0, vectors)
    res, cig, md = c.wanted_cigar_batch(c.idx, c.pac, int(o["w"]), reads, a["regs"], [list(k) for k in a["want"]])
    pe = mode.startswith("pe")
    seqs = [(b"q%d" % (i // 2 if pe else i), b"c" if i % 2 else None, np.asarray(r, dtype=np.uint8), bytes([40 + i % 30]) * len(r) if i % 5 else None)
            for i, r in enumerate(reads)]
    return dict(opt=o, pes=pes, seqs=seqs, vectors=a["regs"], dec=a, res=res, cig=cig, md=md, rg_id=b"rg7")


@pytest.mark.parametrize("mode", ["se", "se-all", "pe", "pe-all"])
def test_slices_through_the_hosts_passes(pkg, real, mode):
    sl = _phase2_slice(pkg, real, mode, 300, seed=3)
    text, _ = _both(pkg, real, sl, mode)
    assert text.count(b"\n") > len(sl["seqs"]) or mode == "pe"


def test_no_read_and_no_wanted_region(pkg, ctx):
    sl = sg.make("se", 0)
    text, off = ctx.sam_text_batch(sl["opt"], ctx.idx, None, [], [], sl["dec"], None, None, None, b"")
    assert text == b"" and off.tolist() == [0]
    for mode in ("se", "pe"):  # every read unmapped: no record, no pool
        b = sg.Builder(np.random.default_rng(8), sg.PE if mode == "pe" else 0)
        for u in range(70):
            name = b"u%d" % u
            for _ in range(2 if mode == "pe" else 1):
                b.add(b.read(name=name), [], n_junk=u % 2)
            if mode == "pe":
                d = np.zeros((), dtype=pkg.PAIRDEC)
                d["extra_flag"] = 1
                b.pd.append(d)
        sl = b.done(b"")
        assert len(sl["res"]) == 0
        text, st = _both(pkg, ctx, sl, "nothing wanted " + mode)
        assert st["lines"] == len(sl["seqs"])
        none = dict(sl, res=None, cig=None, md=None)
        assert ctx.sam_text_batch(*_args(none, ctx.idx))[0] == text


@pytest.mark.parametrize("mode", ["se-all", "pe"])
def test_refusals_leave_the_outputs_untouched(pkg, ctx, mode):
    sl = sg.make(mode, 20, seed=3)
    for what, bad in sg.refusals(sl):
        out = sg.sentinels(len(bad["seqs"]))
        with pytest.raises(pkg.BmhError) as e:
            ctx.sam_text_batch(*_args(bad, ctx.idx), out=out)
        assert e.value.code == pkg.BMH_E_ARG, what
        assert out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all(), what
    _both(pkg, ctx, sl, "after the refusals")  # the context is as good as before


def test_refusals_without_the_resident_tables(pkg):
    sl = sg.make("pe", 12, seed=2)
    idx = sg.refidx()
    c = pkg.Context(0)
    try:
        for setup in ((), ("set_refidx",), ("set_refnames",)):
            c.set_refidx(None), c.set_refnames(None)
            for f in setup:
                getattr(c, f)(idx)
            out = sg.sentinels(len(sl["seqs"]))
            with pytest.raises(pkg.BmhError) as e:
                c.sam_text_batch(*_args(sl, idx), out=out)
            assert e.value.code == pkg.BMH_E_ARG and out["text"].value == 0x5a5a5a5a and (out["text_off"] == -77).all(), setup
        c.set_refidx(idx), c.set_refnames(idx)
        c.idx = idx
        _both(pkg, c, sl, "both resident")
        c.set_refnames(None)
        with pytest.raises(pkg.BmhError):
            c.sam_text_batch(*_args(sl, idx))
    finally:
        c.close()


def test_one_upload_two_waits_and_a_buffer_that_grows(pkg):
    small, large = sg.make("pe-all", 40, seed=6), sg.make("se-all", 1500, seed=6)
    c = pkg.Context(0)
    try:
        c.idx = sg.refidx()
        c.set_refidx(c.idx), c.set_refnames(c.idx)
        for sl in (small, large, small):  # the larger second: the text buffer and the staging grow
            text, st = _both(pkg, c, sl, "sizes")
            n, total, n_w = len(sl["seqs"]), sum(len(v) for v in sl["vectors"]), len(sl["res"])
            pe = bool(int(sl["opt"]["flag"]) & sg.PE)
            cig_words = int((sl["res"]["cigar_off"].astype(np.int64) + sl["res"]["n_cigar"]).max())
            md_bytes = int((sl["res"]["md_off"].astype(np.int64) + sl["res"]["md_len"]).max())
            # the upload as bwamem_hip.h documents it: three offset arrays, the header, rg_id, 4 bytes per read and 8 per region, pd, the
            # regions, the records, the pools as far as the records reach, and the packed reads
            arrays = (3 * 8 * (n + 1) + 144 + len(sl["rg_id"]) + 4 * n + 8 * total + (48 * (n // 2) if pe else 0) + 64 * total + 72 * n_w + 4 * cig_words
                      + md_bytes + len(sg.pack_reads(sl["seqs"])[1]))
            assert 64 * total < st["h2d_bytes"] <= arrays + (8 << 10), (st, arrays)
            assert len(text) < st["d2h_bytes"] <= len(text) + 8 * (n + 1) + (8 << 10), st
            assert st["waits"] == 2 and st["size_ms"] == -1 and st["emit_ms"] == -1
        assert len(pkg.sam_text_batch(*_args(large, c.idx))[0]) > 1 << 20  # (past the buffers' first megabyte)
        c.set_kernel_timing(True)
        _, st = _both(pkg, c, small, "timed")
        assert st["size_ms"] > 0 and st["emit_ms"] > 0
    finally:
        c.close()


# ---------------------------------------------------------------- the switch behind bmh_sam_batch

def _sam_batch(pkg, c, o, pes, id0, vecs, reads, rg_id=b""):
    lib = pkg.lib()
    lib.bmh_sam_batch.restype = C.c_int
    pe = bool(int(o["flag"]) & pg.PE)
    seqs = (pkg._Seq * max(len(reads), 1))()
    keep = []
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        keep.append(r)
        seqs[i] = pkg._Seq(len(r), b"r%d" % (i // 2 if pe else i), b"co" if i % 3 == 0 else None, r.ctypes.data, bytes([35 + i % 40]) * len(r) if i % 4 else None, None)
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


@pytest.mark.parametrize("mode", ["se-all", "pe"])
def test_switch_behind_sam_batch(pkg, real, mode):
    o, pes, id0, reads, vectors = pg.make(mode, n_wanted=300, seed=31)
    c = real
    try:
        t0, r0 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        before = c.last_samtext_stats()
        c.set_samtext_device(True)
        t1, r1 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t1 and r0 == r1
        st = c.last_samtext_stats()
        assert st != before and (st["reads"], st["lines"], st["text_bytes"], st["waits"]) == (len(reads), sum(t.count(b"\n") for t in t0), sum(map(len, t0)), 2), st
        c.set_phase2_device(True)  # on top of the fused passes A and B
        t2, r2 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t2 and r0 == r2 and c.last_phase2_stats()["sessions"] == 1 and c.last_samtext_stats()["reads"] == len(reads)
        # a call that returns before its passes leaves its own statistics, not the previous slice's
        assert _sam_batch(pkg, c, o, pes, id0, [], []) == ([], [])
        st = c.last_samtext_stats()
        assert (st["reads"], st["lines"], st["text_bytes"], st["h2d_bytes"], st["d2h_bytes"], st["waits"], st["size_ms"]) == (0, 0, 0, 0, 0, 0, -1), st
        c.set_phase2_device(False), c.set_samtext_device(False)  # off again: the host's text, the statistics stay
        t3, r3 = _sam_batch(pkg, c, o, pes, id0, vectors, reads, b"grp")
        assert t0 == t3 and r0 == r3 and c.last_samtext_stats() == st
    finally:
        c.set_phase2_device(False), c.set_samtext_device(False)
